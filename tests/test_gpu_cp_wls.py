"""Chambolle-Pock with a per-voxel weighted quadratic data term and a box on the GPU (``-m gpu``): tv_cp_primal_wls through the C-ABI against an
fp64 NumPy restatement of the step (the TEXTBOOK prox (v + tau w x0) / (1 + tau w), clipped, on ``orc.D_T`` of the same inputs -- the kernel
takes v - c (v - x0) with c = tau w / (1 + tau w)), what that form makes exact, the reduce-only residual mode, z-ranges against the whole
volume, the plane-marching form against the one-site form, and ``WeightedChambollePock`` / ``denoise_tv_weighted`` against a NumPy restatement
of Algorithm 1 of Chambolle & Pock 2011 built on ``orc.D`` / ``orc.D_T``: trajectory, residuals, ``run_until``, and that TV fills in unknown
voxels.

Tolerances (tests/test_gpu_cp_prox.py).  With v = x - tau D^T q:
    x_new, x_bar   tol_x = RTOL max(max|v|, max|x0|), RTOL = 1e-5 (fp32) / 1e-11 (fp64): the clamp is 1-Lipschitz, so it adds nothing
    F              tol_x sum w |x_new - x0| + RTOL F: a per-site error of tol_x carried through dF / dx_new = w (x_new - x0), plus the
                   relative rounding of the sum (the "l2" rule of ``fid_tol``)
    R              ``res_tol``: 2 (tol_x / tau) sqrt(N R) + N (tol_x / tau)^2"""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_prox import (DTYPES, LAM, PARITY_SHAPES, PLAIN_KW, RTOL, TAU, WEIGHTINGS, _case_kw, _explicit_pitch, _kw_of, _pads_are_zero,
                              _storage, _tdt, _untouched, _z_channels, gpu_prox, make_inputs, np_project, res_tol)

pytestmark = pytest.mark.gpu

INF = float("inf")
INPUTS = ("q", "x0", "w", "qp", "qn")
EVERYTHING = ("x", "x_bar") + INPUTS


# ------------------------------------------------------------------------------------------------
# the step, restated in fp64 with the textbook formula
# ------------------------------------------------------------------------------------------------
def prox_wls_np(v, x0, w, tau, lo, hi):
    return np.clip((v + tau * w * x0) / (1.0 + tau * w), lo, hi)


def fid_np(x, x0, w):
    return float(0.5 * np.sum(w * (x - x0) ** 2))


def weights_by_thirds(shape, rng, dtype):
    """w by thirds of the sites: 0 (unknown), 1, uniform in [0.25, 2.25]; returns (w, class)"""
    which = rng.integers(0, 3, shape)
    w = np.where(which == 0, 0.0, np.where(which == 1, 1.0, 0.25 + 2.0 * rng.random(shape)))
    return w.astype(dtype), which


def reference(x, gd, x0, w, lo, hi, tau, dtype):
    """everything the checks need, in fp64 from gd = D^T q: the unclamped and the clamped x_new, tol_x, F, R and their tolerances"""
    x, x0, w = (np.asarray(a, dtype=np.float64) for a in (x, x0, w))
    v = x - tau * gd
    xu = (v + tau * w * x0) / (1.0 + tau * w)
    xn = np.clip(xu, lo, hi)
    tol = RTOL[dtype] * max(float(np.max(np.abs(v))), float(np.max(np.abs(x0))))
    fid = fid_np(xn, x0, w)
    res = float(np.sum(((x - xn) / tau) ** 2))
    return dict(x=x, v=v, xu=xu, xn=xn, tol=tol, fid=fid, ftol=tol * float(np.sum(w * np.abs(xn - x0))) + RTOL[dtype] * fid, res=res,
                rtol_res=res_tol(res, tol, tau, x.size), lo=lo, hi=hi)


def boxed(x, gd, x0, w, tau, dtype):
    """shift x and x0 by the (rounded) median of the unclamped x_new, so that the box between its 20th and 80th percentiles contains 0;
    returns (x, x0, lo, hi) with lo, hi representable in dtype"""
    x64, x064, w64 = (np.asarray(a, dtype=np.float64) for a in (x, x0, w))
    s = float(np.round(np.median(((x64 - tau * gd) + tau * w64 * x064) / (1.0 + tau * w64))))
    x, x0 = (x64 - s).astype(dtype), (x064 - s).astype(dtype)
    xu = ((x.astype(np.float64) - tau * gd) + tau * w64 * x0.astype(np.float64)) / (1.0 + tau * w64)
    lo, hi = (float(dtype(p)) for p in np.percentile(xu, (20.0, 80.0)))
    assert lo < 0.0 < hi, (lo, hi)
    return x, x0, lo, hi


@functools.lru_cache(maxsize=None)
def _inputs(shape, scheme, dtype, weighting):
    """x, q, x0 of tests/test_gpu_cp_prox.make_inputs (lambda = 5, tau = 0.3), w by thirds, the box at the 20th / 80th percentile of the
    unclamped x_new with the data shifted so that it contains 0.  Returns (x, q, x0, w, which, kw, ref) with the fp64 restatement ``ref`` of
    the step on exactly these (rounded) arrays."""
    kw = _case_kw(weighting, shape)
    x, q, x0, gd = make_inputs(shape, scheme, dtype, kw)
    w, which = weights_by_thirds(shape, np.random.default_rng(29), dtype)
    x, x0, lo, hi = boxed(x, gd, x0, w, TAU, dtype)
    for a in (x, q, x0, w):
        a.setflags(write=False)
    return x, q, x0, w, which, kw, reference(x, gd, x0, w, lo, hi, TAU, dtype)


def _assert_regimes(what, ref, which):
    """on the reference: clamped low / interior / clamped high and each weight class hold >= 10 % of the sites"""
    shares = (np.mean(ref["xu"] < ref["lo"]), np.mean((ref["xu"] >= ref["lo"]) & (ref["xu"] <= ref["hi"])), np.mean(ref["xu"] > ref["hi"]))
    classes = tuple(np.mean(which == k) for k in range(3))
    print("%s: box [%.4f, %.4f]  clamped low %.3f interior %.3f clamped high %.3f;  w = 0 %.3f  w = 1 %.3f  w in [0.25, 2.25] %.3f" % (
        what, ref["lo"], ref["hi"], *shares, *classes))
    assert min(shares) >= 0.10, shares
    assert min(classes) >= 0.10, classes


def gpu_wls(x, q, x0, w, lo, hi, tau, theta, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None, residual=False,
            null_x_bar=False, x_bar_fill=7.0):
    """tv_cp_primal_wls on local planes [a, b) of the arrays (whole volume by default), halo planes passed by hand.  Returns (x, x_bar, scalar)
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
        t.copy_(torch.as_tensor(np.array(arr)))
        return t

    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), x_bar=img(np.full_like(x[a:b], x_bar_fill)), q=grad(q[a:b]), x0=img(x0[a:b]), w=img(w[a:b]),
               qp=img(q[a - 1:a, cb]) if (a > 0 and g.z_active and drop_halo != "prev") else None,
               qn=img(q[b:b + 1, cf]) if (b < nzg and g.z_active and drop_halo != "next") else None)
    before = {k: _storage(v).clone() for k, v in dev.items() if v is not None}
    if keep is not None:
        keep.update(dev=dev, before=before)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_primal_wls(g.ref, nv.ptr(dev["q"]), nv.ptr(dev["qp"]), nv.ptr(dev["qn"]), nv.ptr(dev["x"]),
                                       None if null_x_bar else nv.ptr(dev["x_bar"]), nv.ptr(dev["x0"]), nv.ptr(dev["w"]), float(lo), float(hi),
                                       float(tau), float(theta), nv.TV_CPP_RESIDUAL if residual else 0, out.data_ptr(), nv.ptr(g.workspace()),
                                       nv.current_stream(g.device)))
    return dev["x"].cpu().numpy(), dev["x_bar"].cpu().numpy(), float(out.item())


def _same_bits(t, before):
    """bit for bit, NaN included (``torch.equal`` calls a poisoned array unequal to itself)"""
    return torch.equal(_storage(t).view(torch.uint8), before.view(torch.uint8))


def _untouched_bits(keep, names):
    for k in names:
        if keep["dev"][k] is not None:
            assert _same_bits(keep["dev"][k], keep["before"][k]), k


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check_step(what, got, ref, theta):
    """x_new, x_bar and F of a step-mode call against the restatement; prints each figure before it asserts"""
    xn, xb, fid = got
    wxb = ref["xn"] + theta * (ref["xn"] - ref["x"])
    ex, eb = float(np.max(np.abs(xn - ref["xn"]))), float(np.max(np.abs(xb - wxb)))
    print("%s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  |dF| %.3e (tol %.3e, F %.6e)" % (what, ex, eb, ref["tol"], abs(fid - ref["fid"]),
                                                                                           ref["ftol"], ref["fid"]))
    assert ex <= ref["tol"], what
    assert eb <= ref["tol"], what
    assert abs(fid - ref["fid"]) <= ref["ftol"], what


# ------------------------------------------------------------------------------------------------
# 1. entry-point parity against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_entry_point_matches_the_restatement(shape, scheme, dtype):
    x, q, x0, w, which, kw, ref = _inputs(shape, scheme, dtype, "plain")
    _assert_regimes("plain %s %s %s" % (scheme, shape, np.dtype(dtype).name), ref, which)
    for theta in (0.0, 0.37, 1.0):
        keep = {}
        got = gpu_wls(x, q, x0, w, ref["lo"], ref["hi"], TAU, theta, scheme, dtype, kw, keep=keep)
        assert got[0].dtype == dtype and got[1].dtype == dtype
        _check_step("plain %s theta %g" % (scheme, theta), got, ref, theta)
        if theta == 0.0:
            np.testing.assert_array_equal(got[1], got[0])           # x_bar = x_new exactly
        _untouched(keep, INPUTS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_entry_point_under_the_four_weightings_and_explicit_pitch(scheme, dtype):
    shape = (3, 2, 16, 20)
    for weighting in WEIGHTINGS:
        x, q, x0, w, which, kw, ref = _inputs(shape, scheme, dtype, weighting)
        _assert_regimes("%s %s %s" % (weighting, scheme, np.dtype(dtype).name), ref, which)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            keep = {}
            got = gpu_wls(x, q, x0, w, ref["lo"], ref["hi"], TAU, 1.0, scheme, dtype, kw, pitch=pitch, keep=keep)
            _check_step("%s %s pitch %r" % (weighting, scheme, pitch), got, ref, 1.0)
            _untouched(keep, INPUTS)
            if pitch != (0, 0):
                _pads_are_zero(keep["dev"]["x"])
                _pads_are_zero(keep["dev"]["x_bar"])


# ------------------------------------------------------------------------------------------------
# 2. what the form of the prox makes exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bounds_unknown_sites_and_fixed_points_are_exact(scheme, dtype):
    for shape in PARITY_SHAPES:
        x, q, x0, w, which, kw, ref = _inputs(shape, scheme, dtype, "plain")
        lo, hi, tol = ref["lo"], ref["hi"], ref["tol"]
        low, high = ref["xu"] < lo - tol, ref["xu"] > hi + tol          # (nearer to a bound the rounding of v decides the side)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            keep = {}
            xn, xb, fid = gpu_wls(x, q, x0, w, lo, hi, TAU, 1.0, scheme, dtype, kw, pitch=pitch, keep=keep)
            print("%s %s pitch %r: %d / %d of %d sites clamped low / high by more than tol; range of x_new [%.6f, %.6f] in [%.6f, %.6f]" % (
                scheme, shape, pitch, low.sum(), high.sum(), low.size, xn.min(), xn.max(), lo, hi))
            assert low.sum() >= 0.10 * low.size and high.sum() >= 0.10 * high.size
            assert np.all(xn >= dtype(lo)) and np.all(xn <= dtype(hi))         # every output lies in the box
            assert np.array_equal(_bits(xn[low]), _bits(np.full(int(low.sum()), lo, dtype=dtype)))
            assert np.array_equal(_bits(xn[high]), _bits(np.full(int(high.sum()), hi, dtype=dtype)))
            assert np.isfinite(fid) and np.all(np.isfinite(xb))
            _pads_are_zero(keep["dev"]["x"])                           # the whole allocation: what is not a voxel is a pad
            _pads_are_zero(keep["dev"]["x_bar"])
            # q = 0 and w = 0: x_new = clamp(x), whatever x0 holds
            zq, zw = np.zeros_like(q), np.zeros_like(w)
            for l, h in ((lo, hi), (-INF, INF), (0.0, INF), (-INF, 0.0)):
                xn, xb, fid = gpu_wls(x, zq, x0, zw, l, h, TAU, 1.0, scheme, dtype, kw, pitch=pitch)
                want = np.clip(x, dtype(l), dtype(h))
                assert np.array_equal(_bits(xn), _bits(want)), (l, h)
                assert fid == 0.0
            # x = x0 = a constant inside the box, q = 0, any w: a fixed point bit for bit, residual exactly 0
            for const in (0.75 * hi, 0.5 * lo, 0.0, hi, lo):
                c = np.full(shape, const, dtype=dtype)
                xn, xb, fid = gpu_wls(c, zq, c, w, lo, hi, TAU, 1.0, scheme, dtype, kw, pitch=pitch)
                assert np.array_equal(_bits(xn), _bits(c)) and np.array_equal(_bits(xb), _bits(c)) and fid == 0.0, const
                assert gpu_wls(c, zq, c, w, lo, hi, TAU, 1.0, scheme, dtype, kw, pitch=pitch, residual=True)[2] == 0.0, const


# ------------------------------------------------------------------------------------------------
# 3. w = 1 without a box is the quadratic term of the accelerated solver's kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_unit_weights_without_a_box_agree_with_tv_cp_primal_accel(scheme, dtype):
    for shape in PARITY_SHAPES:
        x, q, x0, gd = make_inputs(shape, scheme, dtype, PLAIN_KW)
        ones = np.ones(shape, dtype=dtype)
        ref = reference(x, gd, x0, ones, -INF, INF, TAU, dtype)
        for theta in (0.0, 0.37, 1.0):
            a = gpu_prox(x, q, x0, "l2", TAU, theta, scheme, dtype, PLAIN_KW, entry="accel")
            p = gpu_wls(x, q, x0, ones, -INF, INF, TAU, theta, scheme, dtype, PLAIN_KW)
            print("%s %s theta %g: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  fid rel %.3e" % (
                scheme, shape, theta, np.max(np.abs(p[0] - a[0])), np.max(np.abs(p[1] - a[1])), ref["tol"], abs(p[2] / a[2] - 1.0)))
            assert float(np.max(np.abs(p[0] - a[0]))) <= ref["tol"] and float(np.max(np.abs(p[1] - a[1]))) <= ref["tol"]
            assert abs(p[2] - a[2]) <= ref["ftol"]
            _check_step("%s %s w = 1" % (scheme, shape), p, ref, theta)


# ------------------------------------------------------------------------------------------------
# 4. residual mode: reduce-only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_residual_mode_reduces_and_writes_nothing(scheme, dtype):
    shape = (3, 2, 16, 20)
    x, q, x0, w, _, kw, ref = _inputs(shape, scheme, dtype, "plain")
    lo, hi = ref["lo"], ref["hi"]
    vals = {}
    for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
        for null_x_bar in (False, True):
            keep = {}
            # theta is ignored: a value the step mode refuses; x_bar is poisoned
            _, _, res = gpu_wls(x, q, x0, w, lo, hi, TAU, 5.0, scheme, dtype, kw, pitch=pitch, keep=keep, residual=True, null_x_bar=null_x_bar,
                                x_bar_fill=float("nan"))
            _untouched_bits(keep, EVERYTHING)
            vals[(pitch, null_x_bar)] = res
            assert abs(res - ref["res"]) <= ref["rtol_res"], (pitch, null_x_bar, res, ref["res"], ref["rtol_res"])
        assert vals[(pitch, True)] == vals[(pitch, False)]
    # what a step would change: sum (x_before - x_after)^2 / tau^2
    xn, _, _ = gpu_wls(x, q, x0, w, lo, hi, TAU, 1.0, scheme, dtype, kw)
    stepped = float(np.sum((x.astype(np.float64) - xn.astype(np.float64)) ** 2)) / TAU ** 2
    print("%s %s: R %.12e restated %.12e from a step %.12e (tol %.3e)" % (scheme, np.dtype(dtype).name, vals[((0, 0), False)], ref["res"], stepped,
                                                                          ref["rtol_res"]))
    assert abs(vals[((0, 0), False)] - stepped) <= ref["rtol_res"]


# ------------------------------------------------------------------------------------------------
# 5. z-ranges: planes [a, b) with hand-made halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
Z_SHAPE = (5, 2, 16, 20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_z_ranges_equal_the_whole_volume(scheme, dtype):
    theta = 0.37
    x, q, x0, w, _, kw, ref = _inputs(Z_SHAPE, scheme, dtype, "plain")
    lo, hi = ref["lo"], ref["hi"]
    wxn, wxb, wfid = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, kw)
    wres = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, kw, residual=True)[2]
    for cut in ((0, 1, 5), (0, 2, 5), (0, 1, 4, 5)):
        fids, ress = [], []
        for a, b in zip(cut[:-1], cut[1:]):
            keep = {}
            xn, xb, fid = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, kw, z_range=(a, b), keep=keep)
            np.testing.assert_array_equal(xn, wxn[a:b], err_msg="x, cut %r planes [%d, %d)" % (cut, a, b))
            np.testing.assert_array_equal(xb, wxb[a:b], err_msg="x_bar, cut %r planes [%d, %d)" % (cut, a, b))
            _untouched(keep, INPUTS)                               # q, x0, w and the halo planes
            fids.append(fid)
            keep = {}
            ress.append(gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, kw, z_range=(a, b), keep=keep, residual=True)[2])
            _untouched(keep, EVERYTHING)
        print("cut %r: F parts sum %.17g whole %.17g; R parts sum %.17g whole %.17g" % (cut, sum(fids), wfid, sum(ress), wres))
        assert abs(sum(fids) - wfid) <= 1e-13 * wfid, cut           # the same fp64 terms in another order
        assert abs(sum(ress) - wres) <= 1e-13 * wres, cut


@pytest.mark.parametrize("scheme", SCHEMES)
def test_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    x, q, x0, w, _, kw, ref = _inputs(Z_SHAPE, scheme, np.float32, "plain")
    # the adjoint of a forward difference reads the previous slab, of a backward difference the next one (central, hybrid: both)
    sides = {"upwind": ("prev",), "downwind": ("next",)}.get(scheme, ("prev", "next"))
    for side in sides:
        for residual in (False, True):
            keep = {}
            with pytest.raises(ValueError, match=r"halo.*code -2"):
                gpu_wls(x, q, x0, w, ref["lo"], ref["hi"], TAU, 1.0, scheme, np.float32, kw, z_range=(1, 4), keep=keep, drop_halo=side,
                        residual=residual)
            torch.cuda.synchronize()
            _untouched(keep, EVERYTHING)


# ------------------------------------------------------------------------------------------------
# 6. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
MARCH_SHAPE = (2, 2, 1024, 1024)


@functools.lru_cache(maxsize=1)
def _march_inputs(scheme):
    """x and q of tests/test_gpu_cp_kl._march_inputs (before its lowering of x), x0 = x + uniform noise, w by thirds, the box at the 20th / 80th
    percentile with the data shifted; the restatement of the step on them"""
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, MARCH_SHAPE[0], MARCH_SHAPE[1], **PLAIN_KW)
    x = 60.0 * rng.random(MARCH_SHAPE, dtype=np.float32)
    q = LAM * (rng.random((MARCH_SHAPE[0], nd) + MARCH_SHAPE[1:], dtype=np.float32) - 0.5)
    x0 = x + np.float32(2.4) * (2.0 * rng.random(MARCH_SHAPE, dtype=np.float32) - 1.0)
    w, which = weights_by_thirds(MARCH_SHAPE, rng, np.float32)
    gd = orc.D_T(q.astype(np.float64), scheme, **PLAIN_KW)
    x, x0, lo, hi = boxed(x, gd, x0, w, TAU, np.float32)
    return x, q, x0, w, which, reference(x, gd, x0, w, lo, hi, TAU, np.float32)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_marching_form_equals_one_site_form(scheme, tvopt):
    dtype, theta = np.float32, 0.37
    x, q, x0, w, which, ref = _march_inputs(scheme)
    _assert_regimes("%s marching" % scheme, ref, which)
    lo, hi, tol = ref["lo"], ref["hi"], ref["tol"]
    march = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, PLAIN_KW)
    march_res = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    tvopt("TV_NO_MARCH", 1)
    site = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, PLAIN_KW)
    site_res = gpu_wls(x, q, x0, w, lo, hi, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    print("%s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  F %.9e / %.9e (tol %.3e)  R %.9e / %.9e / restated %.9e (tol %.3e)  sites on a bound %.3f" % (
        scheme, np.max(np.abs(march[0] - site[0])), np.max(np.abs(march[1] - site[1])), tol, march[2], site[2], ref["ftol"], march_res, site_res,
        ref["res"], ref["rtol_res"], np.mean((site[0] == dtype(lo)) | (site[0] == dtype(hi)))))
    assert float(np.max(np.abs(march[0] - site[0]))) <= tol
    assert float(np.max(np.abs(march[1] - site[1]))) <= tol
    assert abs(march[2] - site[2]) <= ref["ftol"]
    assert abs(march_res - site_res) <= ref["rtol_res"]
    assert np.isfinite(march[2]) and march[2] > 0.0 and np.isfinite(march_res) and march_res > 0.0
    for got in (march, site):
        assert np.all(got[0] >= dtype(lo)) and np.all(got[0] <= dtype(hi))
    # and both are the restatement's step, in both modes
    _check_step("%s marching" % scheme, march, ref, theta)
    _check_step("%s one-site" % scheme, site, ref, theta)
    assert abs(march_res - ref["res"]) <= ref["rtol_res"] and abs(site_res - ref["res"]) <= ref["rtol_res"]


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 1, theta = 1) and of its optimality residuals
# ------------------------------------------------------------------------------------------------
REG = 0.5
TRAJ_SHAPES = [(1, 1, 24, 28), (3, 2, 16, 20)]
N_TRAJ = 60
CASES = ("inpaint", "box", "shift")


@functools.lru_cache(maxsize=None)
def clean_phantom(shape):
    """2 with a centred square of 20"""
    c = np.full(shape, 2.0)
    ny, nx = shape[2:]
    c[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 20.0
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def problem(shape, case):
    """(x0, w, lower, upper): the phantom plus N(0, 1) noise, rounded to fp32 so that both precisions see the same data.
    "inpaint": 30 % of the sites unknown (w = 0) and zero-filled, the others w = 1, no box.  "box": w uniform in [0.25, 2.25], the box [0, 18].
    "shift": those weights with lower = 1 and no upper bound -- a box without 0, which the solver shifts.
    "inpaint_box" (tests/test_gpu_thin_slabs.py; not one of ``CASES``): the data of "inpaint" with the box of "box"."""
    rng = np.random.default_rng(0)
    x0 = (clean_phantom(shape) + rng.standard_normal(shape)).astype(np.float32).astype(np.float64)
    if case in ("inpaint", "inpaint_box"):
        known = rng.random(shape) >= 0.3
        x0[~known] = 0.0
        out = (x0, known, None, None) if case == "inpaint" else (x0, known, 0.0, 18.0)
    else:
        w = (0.25 + 2.0 * rng.random(shape)).astype(np.float32).astype(np.float64)
        out = (x0, w, 0.0, 18.0) if case == "box" else (x0, w, 1.0, None)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def _bounds(lower, upper):
    return (-INF if lower is None else lower), (INF if upper is None else upper)


def _steps_of(shape, scheme):
    s = 1.0 / np.sqrt(orc.normal_spectral_bound(scheme, shape, **_kw_of(shape)))
    return s, s


def np_residuals(x, q, x0, w, lo, hi, lam, scheme, kw, tau, sigma):
    """the dict of ``residuals()``, and the absolute rounding floor of R_x in fp64: x - x_new carries an error of a few eps (|v| + |x0|) per
    site, so R_x carries 2 sqrt(R_x E) + E with E = sum (4 eps (|v| + |x0|) / tau)^2 -- what the textbook formula leaves of R_x at a fixed
    point, where the kernel's form gives 0"""
    Dx = orc.D(x, scheme, **kw)
    rq = float(np.sum((q - np_project(q + sigma * Dx, lam)) ** 2)) / sigma ** 2
    v = x - tau * orc.D_T(q, scheme, **kw)
    xn = prox_wls_np(v, x0, w, tau, lo, hi)
    rx = float(np.sum(((x - xn) / tau) ** 2))
    e = float(np.sum((4.0 * np.finfo(np.float64).eps * (np.abs(v) + np.abs(x0)) / tau) ** 2))
    return {"x": rx, "q": rq, "total": rx + rq, "tv": float(orc.compute_L21_norm(Dx)), "fid": fid_np(x, x0, w)}, 2.0 * np.sqrt(rx * e) + e


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, case, n_iter):
    """(x, loss, q, loss tolerance of an fp32 run) after n_iter iterations from clamp(x0), on the problem AS STATED (no shift).  The fp32 loss
    tolerance of iteration k is 1e-5 |loss| + sum_i g_i (1e-5 |x_i| + 2e-3) with g_i = w_i |x_i - x0_i|: the project's fp32 tolerance of the
    iterate (rtol 1e-5, atol 2e-3) carried through dF / dx, as in tests/test_gpu_cp_kl.py."""
    x0, w, lower, upper = problem(shape, case)
    w = np.asarray(w, dtype=np.float64)
    lo, hi = _bounds(lower, upper)
    kw, lam = _kw_of(shape), REG
    tau, sigma = _steps_of(shape, scheme)
    x = np.clip(x0, lo, hi)
    xb = x.copy()
    q = np.zeros_like(orc.D(x0, scheme, **kw))
    loss, ltol = np.zeros(n_iter), np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project(q + sigma * Dxb, lam)
        xn = prox_wls_np(x - tau * orc.D_T(q, scheme, **kw), x0, w, tau, lo, hi)
        xb = 2.0 * xn - x
        x = xn
        loss[k] = fid_np(x, x0, w) + lam * orc.compute_L21_norm(Dxb)
        ltol[k] = 1e-5 * abs(loss[k]) + float(np.sum(w * np.abs(x - x0) * (1e-5 * np.abs(x) + 2e-3)))
    return x, loss, q, ltol


def _solver(pytv, shape, dtype, scheme, case, **how):
    x0, w, lower, upper = problem(shape, case)
    wt = torch.as_tensor(np.array(w)).cuda()
    if wt.dtype != torch.bool:
        wt = wt.to(_tdt(dtype))
    return pytv.solvers.WeightedChambollePock(torch.as_tensor(x0.astype(dtype)).cuda(), REG, wt, lower=lower, upper=upper, scheme=scheme,
                                              **_kw_of(shape), **how)


# ------------------------------------------------------------------------------------------------
# 7. solver trajectory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme, case):
    import pytv
    x0, w, lower, upper = problem(shape, case)
    lo, hi = _bounds(lower, upper)
    wx, wloss, _, _ = np_trajectory(shape, scheme, case, N_TRAJ)
    cp = _solver(pytv, shape, np.float64, scheme, case)
    assert cp.it == 0 and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape)) and cp.tau == cp.sigma == 1.0 / np.sqrt(cp.L2)
    assert cp.shift == (1.0 if case == "shift" else 0.0) and cp.lower == lo - cp.shift and cp.upper == hi - cp.shift
    assert cp.lower <= 0.0 <= cp.upper
    assert torch.equal(cp.x, cp.x0.clamp(cp.lower, cp.upper)) and torch.equal(cp.x_bar, cp.x) and cp.w.dtype == torch.float64
    loss = cp.run(N_TRAJ)
    x = cp.result().cpu().numpy()
    on = (np.mean(x == lo), np.mean(x == hi))
    print("%s %s %s: loss rel %.3e  max|dx| %.3e  sites on the lower / upper bound %.3f / %.3f (restatement %.3f / %.3f)" % (
        scheme, shape, case, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx)), *on, np.mean(wx == lo), np.mean(wx == hi)))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(x0)))
    assert cp.it == N_TRAJ and np.all(x >= lo) and np.all(x <= hi)
    if case == "box":
        assert on[1] >= 0.15                                          # the square sits on the upper bound, exactly
    if case == "shift":
        assert on[0] > 0.0                                            # (restatement: 1 - 4.5 % of the sites)
    # run(25); run(35) is run(60) bit for bit; reset() reproduces the run; record_loss=False returns nothing and computes the same
    two = _solver(pytv, shape, np.float64, scheme, case)
    np.testing.assert_array_equal(np.concatenate([two.run(25), two.run(35)]), loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.x_bar, cp.x_bar) and torch.equal(two.q, cp.q)
    two.reset()
    assert two.it == 0 and torch.equal(two.x, two.x0.clamp(two.lower, two.upper)) and torch.equal(two.x_bar, two.x) and not bool(two.q.any())
    assert two.run(N_TRAJ, record_loss=False) is None
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.q, cp.q)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme, case):
    """against the fp64 restatement on the same data (rounded to fp32 beforehand): result rtol 1e-5, atol 2e-3 (the project's fp32 figures);
    loss to that tolerance carried through dF / dx (``np_trajectory``)"""
    import pytv
    lo, hi = _bounds(*problem(shape, case)[2:])
    wx, wloss, _, ltol = np_trajectory(shape, scheme, case, N_TRAJ)
    cp = _solver(pytv, shape, np.float32, scheme, case)
    assert cp.w.dtype == torch.float32
    loss = cp.run(N_TRAJ)
    x = cp.result().cpu().numpy()
    print("%s %s %s: max |dloss| / tol %.3e  max|dx| %.3e" % (scheme, shape, case, np.max(np.abs(loss - wloss) / ltol), np.max(np.abs(x - wx))))
    assert np.all(np.isfinite(loss))
    assert np.all(np.abs(loss - wloss) <= ltol)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)
    assert np.all(x >= lo) and np.all(x <= hi)


# ------------------------------------------------------------------------------------------------
# 8. certificate and stopping
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_residuals_against_the_restatement(shape, scheme, case):
    import pytv
    x0, w, lower, upper = problem(shape, case)
    w = np.asarray(w, dtype=np.float64)
    lo, hi = _bounds(lower, upper)
    kw = _kw_of(shape)
    tau, sigma = _steps_of(shape, scheme)
    start = (np.clip(x0, lo, hi), None, np.zeros_like(orc.D(x0, scheme, **kw)), None)
    cp = _solver(pytv, shape, np.float64, scheme, case)
    done = 0
    for n in (0, 1, 30):
        if n > done:
            cp.run(n - done)
            done = n
        wx, _, wq, _ = np_trajectory(shape, scheme, case, n) if n else start
        want, floor = np_residuals(wx, wq, x0, w, lo, hi, REG, scheme, kw, tau, sigma)
        state = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
        got = cp.residuals()
        print("%s %s %s after %d: %r  restated %r  (fp64 floor of R_x %.3e)" % (scheme, shape, case, n, got, want, floor))
        assert sorted(got) == ["fid", "q", "total", "tv", "x"] and got["total"] == got["x"] + got["q"]
        for k in ("q", "tv", "fid"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=0, err_msg="%s after %d" % (k, n))
        np.testing.assert_allclose(got["x"], want["x"], rtol=1e-9, atol=floor, err_msg="x after %d" % n)
        assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q)))
        if n == 0:
            assert got["x"] == 0.0 and got["total"] == cp.initial_residual() > 0.0      # x = clamp(x0), q = 0: F's block is at rest
    np.testing.assert_allclose(cp.initial_residual(), np_residuals(*start[0:3:2], x0, w, lo, hi, REG, scheme, kw, tau, sigma)[0]["total"], rtol=1e-9)


@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_run_until_converges_and_fills_the_unknown_sites(shape, scheme):
    """This file's NumPy restatement (30 % unknown, zero fill, default steps, reg 0.5), the four cases in the order they run: the relative
    residual is 2.1e-2 / 2.5e-2 / 8.2e-3 / 1.1e-2 after 100 iterations and 1.1e-2 / 4.0e-3 / 6.0e-4 / 6.1e-4 after 200 (so the first case
    needs a little more than 200); the RMS error at the unknown sites against the clean phantom is 0.59 / 1.49 / 1.59 / 2.27 after 200
    where the zero fill has 9.86 / 10.66 (0.06 - 0.21 of it)"""
    import pytv
    x0, known, _, _ = problem(shape, "inpaint")
    clean = clean_phantom(shape)
    cp = _solver(pytv, shape, np.float64, scheme, "inpaint")
    r0 = cp.initial_residual()
    loss, info = cp.run_until(1e-2, 400)
    out = cp.result().cpu().numpy()
    rms = lambda a: float(np.sqrt(np.mean((a[~known] - clean[~known]) ** 2)))
    print("%s %s: %r;  RMS error at the unknown sites: zero fill %.3f  inpainted %.3f  ratio %.3f" % (scheme, shape, info, rms(x0), rms(out),
                                                                                                    rms(out) / rms(x0)))
    assert info["converged"] is True and 50 < info["iterations"] < 400 and info["iterations"] % 10 == 0
    assert len(loss) == info["iterations"] == cp.it and np.all(np.isfinite(loss))
    assert info["initial"] == r0 and info["residuals"]["total"] <= 1e-2 ** 2 * r0
    assert info["relative"] == np.sqrt(cp.residuals()["total"] / r0)
    assert sorted(info) == ["converged", "initial", "iterations", "relative", "residuals"]
    assert rms(out) < 0.5 * rms(x0)


# ------------------------------------------------------------------------------------------------
# 9. fixed points, constructor and front-end
# ------------------------------------------------------------------------------------------------
def test_run_until_on_a_constant_image_inside_the_box_returns_at_once():
    import pytv
    shape = (2, 2, 8, 12)
    w = torch.rand(shape, device="cuda", dtype=torch.float64) + 0.1
    for dtype in (torch.float32, torch.float64):
        for scheme in SCHEMES:
            for lower, upper in ((None, None), (0.0, 10.0), (5.0, 9.0), (7.0, 7.0)):
                cp = pytv.solvers.WeightedChambollePock(torch.full(shape, 7.0, dtype=dtype, device="cuda"), 1.0, w.to(dtype), lower=lower,
                                                        upper=upper, scheme=scheme, reg_time=0.5)
                loss, info = cp.run_until(1e-3, 100)
                assert info["converged"] is True and info["iterations"] == 0 == cp.it and info["initial"] == 0.0 and info["relative"] == 0.0
                assert len(loss) == 0 and cp.shift == (0.0 if lower in (None, 0.0) else lower)
                assert bool((cp.result() == 7.0).all())
                cp.run(5)                                              # and stays there, bit for bit
                assert bool((cp.result() == 7.0).all()) and not bool(cp.q.any())


def test_constructor_refuses_bad_arguments():
    import pytv
    cls = pytv.solvers.WeightedChambollePock
    shape = (1, 1, 24, 28)
    x0n, wn, _, _ = problem(shape, "box")
    for dtype in (np.float32, np.float64):
        x0, w = torch.as_tensor(x0n.astype(dtype)).cuda(), torch.as_tensor(wn.astype(dtype)).cuda()
        for bad_shape in ((1, 1, 24, 27), (1, 24, 28), (24, 28)):
            with pytest.raises(ValueError, match="shape"):
                cls(x0, 1.0, torch.ones(bad_shape, device="cuda"))
        for bad_value in (-1.0, -1e-30, float("nan"), INF, -INF):
            bad = w.clone()
            bad[0, 0, 5, 7] = bad_value
            with pytest.raises(ValueError, match="weights must be finite"):
                cls(x0, 1.0, bad)
        for bad_value in (float("nan"), INF, -INF):
            bad = x0.clone()
            bad[0, 0, 5, 7] = bad_value
            with pytest.raises(ValueError, match="x0 must be finite"):
                cls(bad, 1.0, w)
        with pytest.raises(ValueError, match="lower"):
            cls(x0, 1.0, w, lower=2.0, upper=1.0)
        with pytest.raises(ValueError, match="lower"):
            cls(x0, 1.0, w, lower=float("nan"))
        with pytest.raises(ValueError, match="zero everywhere"):
            cls(x0, 1.0, torch.zeros_like(w))
        with pytest.raises(ValueError, match="zero everywhere"):
            cls(x0, 1.0, torch.zeros(shape, dtype=torch.bool, device="cuda"))
        huge = w.clone()
        huge[0, 0, 3, 3] = float(np.finfo(dtype).max) / 2.0
        with pytest.raises(ValueError, match="not finite"):
            cls(x0, 1.0, huge, tau=4.0)
        cls(x0, 1.0, huge, tau=1.0)
        with pytest.raises(ValueError, match="bool or floating"):
            cls(x0, 1.0, torch.ones(shape, dtype=torch.int32, device="cuda"))
    L2 = 8.0
    with pytest.raises(ValueError, match="tau"):
        cls(x0, 1.0, w, scheme="upwind", tau=1.0, sigma=(1.0 + 1e-9) / L2)
    ok = cls(x0, 1.0, w, scheme="upwind", tau=1.0, sigma=1.0 / L2)
    assert ok.L2 == L2 and (ok.tau, ok.sigma) == (1.0, 1.0 / L2)
    assert cls(x0, 1.0, w, scheme="upwind", sigma=0.25).tau == 1.0 / (L2 * 0.25)
    # a bool mask is stored as 1 / 0 in the layout and dtype of x0; a NumPy array is taken as well
    mask = wn > 1.0
    for m in (torch.as_tensor(mask).cuda(), mask):
        cp = cls(x0, 1.0, m, pitch=(32, 24 * 32 + 8))
        assert cp.w.dtype == x0.dtype and cp.w.stride() == cp.x0.stride() and torch.equal(cp.w.cpu(), torch.as_tensor(mask).to(x0.dtype))
        _pads_are_zero(cp.w)
        cp.run(3)
        _pads_are_zero(cp.x)
        _pads_are_zero(cp.x_bar)


def test_denoise_tv_weighted_front_end():
    import pytv
    shape = (1, 1, 24, 28)
    x0n, known, _, _ = problem(shape, "inpaint")
    img, mask = x0n[0, 0].astype(np.float32), np.array(known[0, 0])        # (a writable copy: the cached problem is read-only)
    vol = torch.as_tensor(img.reshape(shape)).cuda()
    out = pytv.denoise_tv_weighted(img, mask, 0.5)
    ref = pytv.solvers.WeightedChambollePock(vol, 0.5, torch.as_tensor(np.array(known)).cuda(), scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-2, 400, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] % 10 == 0 and info["iterations"] < 400
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == img.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # never converges: exactly 40 iterations, the solver's run(40), with bounds, float weights and a step of the caller's
    wf = (0.5 + mask).astype(np.float32)
    out = pytv.denoise_tv_weighted(img, wf, 0.5, 1.0, 18.0, rel_res=0.0, max_num_iter=40, scheme="hybrid", tau=0.2)
    ref = pytv.solvers.WeightedChambollePock(vol, 0.5, torch.as_tensor(wf.reshape(shape)).cuda(), lower=1.0, upper=18.0, scheme="hybrid", tau=0.2)
    ref.run(40)
    assert ref.shift == 1.0
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    assert out.min() == 1.0 and out.max() == 18.0                        # the bounds hold exactly, and both are reached
    # torch in -> device tensor out, fp64 stays fp64; 3-D input is a stack with a z axis; 4-D and a wrong mask shape are refused
    t = pytv.denoise_tv_weighted(vol[0, 0].double(), torch.as_tensor(mask).cuda(), 0.5, rel_res=0.0, max_num_iter=10)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.shape == vol.shape[2:]
    stack, masks = np.stack([img, img[::-1], img]), np.stack([mask, mask[::-1], mask])
    out3 = pytv.denoise_tv_weighted(stack, masks, 0.5, lower=0.0, rel_res=0.0, max_num_iter=10)
    ref3 = pytv.solvers.WeightedChambollePock(torch.as_tensor(stack.reshape(3, 1, 24, 28).copy()).cuda(), 0.5,
                                              torch.as_tensor(masks.reshape(3, 1, 24, 28).copy()).cuda(), lower=0.0, scheme="upwind",
                                              reg_z_over_reg=1.0)
    ref3.run_until(0.0, 10)
    assert out3.shape == stack.shape and out3.dtype == np.float32 and out3.min() >= 0.0
    np.testing.assert_array_equal(out3, ref3.result().cpu().numpy().reshape(stack.shape))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.denoise_tv_weighted(np.zeros((1, 1, 8, 8), dtype=np.float32), np.ones((1, 1, 8, 8), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        pytv.denoise_tv_weighted(img, mask[:, :-1])
