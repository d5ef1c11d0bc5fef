"""Spatially adaptive TV (a per-voxel weight g on the TV term) on the GPU (``-m gpu``): tv_cp_dual_wtv and tv_dual_gap_wtv through the C-ABI
against fp64 NumPy restatements built on ``orc.D`` / ``orc.D_T`` (textbook formulas: ``np.where`` on |v| > r with a division), the invariants
of the projection (inside the ball: v bit for bit; g = 0: q = 0; never beyond the radius), constant g against tv_cp_dual, z-ranges against
the whole volume, the plane-marching form against the one-site form, and ``AdaptiveTVChambollePock`` / ``denoise_tv_adaptive`` /
``edge_stopping_weights`` against a NumPy restatement of Algorithm 2 of Chambolle & Pock 2011 with the per-site radius -- trajectory, certified
stop, and that the model does what it is for: a protected region is left alone, an edge-stopping weight keeps an edge.

Tolerances are the project's (tests/test_gpu_cp_huber.py): arrays to RTOL[dtype] * max|ref| with RTOL 1e-5 (fp32) / 1e-11 (fp64), scalars to
RTOL[dtype] * sum |terms| of the sum they are; trajectories: fp64 loss rtol 1e-10 and result 1e-9 * max|x0|, fp32 loss rtol 1e-5 and result
rtol 1e-5 / atol 2e-3 on fp32-rounded input; a feasible pair's gap >= -16 eps_dtype * primal."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_prox import (PARITY_SHAPES, WEIGHTINGS, _case_kw, _explicit_pitch, _pads_are_zero, _storage, _untouched, _z_channels,
                              make_inputs)
from test_gpu_cp_huber import STOP_SHAPES, TRAJ_SHAPES, WS_FILL, _geometry, _kw_of, _tdt, _uploaders, _ws_beyond_the_partials_untouched, noisy_square

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
DTYPES = [np.float64, np.float32]
PLAIN_KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
LAM = 5.0                      # the radius of make_inputs' q
SIGMA = 0.1                    # x of make_inputs is 0..60: sigma |D x| is a few units, |v| = |q + sigma D x| a few units up to ~10, against
                               # radii LAM g in (0, 5) and (5, 15): both sides of |v| = r hold well over 10 % of the g > 0 sites (asserted)


def make_g(shape, dtype, seed=23):
    """a third of the sites exactly 0, a third in (0, 1), a third in (1, 3), from a fixed seed"""
    rng = np.random.default_rng(seed)
    kind, u = rng.integers(0, 3, shape), rng.random(shape)
    return np.where(kind == 0, 0.0, np.where(kind == 1, 0.05 + 0.9 * u, 1.0 + 2.0 * u)).astype(dtype)


# ------------------------------------------------------------------------------------------------
# the two kernels, restated in fp64
# ------------------------------------------------------------------------------------------------
def np_project_r(v, r):
    """v where |v|_2 <= r, v r / |v|_2 beyond; r per site (broadcast over the channel axis)"""
    n = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
    r = np.asarray(r, dtype=np.float64)[:, None]
    return np.where(n > r, v * (r / np.where(n > 0.0, n, 1.0)), v)


def ref_dual(x, q, g, sigma, lam, scheme, kw):
    """(q_new, sum g |D x|, v, |v|, r) in fp64"""
    g = np.asarray(g, dtype=np.float64)
    Dx = orc.D(np.asarray(x, dtype=np.float64), scheme, **kw)
    v = np.asarray(q, dtype=np.float64) + sigma * Dx
    n = np.sqrt(np.sum(Dx * Dx, axis=1))
    return np_project_r(v, lam * g), float(np.sum(g * n)), v, np.sqrt(np.sum(v * v, axis=1)), lam * g


def ref_gap(x, q, x0, g, lam, scheme, kw):
    """(sum g |D x|, 1/2 |x - x0|^2, gap, sum |terms of the gap|) in fp64, the gap site by site as
    1/2 (x - x0 + D^T q)^2 + (lam g |D x| - <q, D x>)"""
    x, q, x0, g = (np.asarray(a, dtype=np.float64) for a in (x, q, x0, g))
    Dx = orc.D(x, scheme, **kw)
    r = x - x0 + orc.D_T(q, scheme, **kw)
    gn = g * np.sqrt(np.sum(Dx * Dx, axis=1))
    dot = np.sum(q * Dx, axis=1)
    gap = np.sum(0.5 * r * r) + np.sum(lam * gn - dot)
    terms = np.sum(0.5 * r * r) + np.sum(lam * gn + np.abs(dot))
    return float(np.sum(gn)), float(0.5 * np.sum((x - x0) ** 2)), float(gap), float(terms)


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, scheme, dtype, weighting):
    kw = _case_kw(weighting, shape)
    x, q, x0, _ = make_inputs(shape, scheme, dtype, kw)
    g = make_g(shape, dtype)
    for a in (x, q, x0, g):
        a.setflags(write=False)
    return x, q, x0, g, kw


def gpu_dual(x, q, g, sigma, lam, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None):
    """tv_cp_dual_wtv (g an array) or tv_cp_dual (g None) on local planes [a, b) (whole volume by default), halo planes of x passed by hand.
    Returns (q after the call, the scalar).  keep: receives the device tensors, copies of their storage made before the call, and the workspace
    (filled with WS_FILL before the call).  drop_halo: "prev" / "next" -- pass NULL for that halo plane."""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    geo = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(geo)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]), gw=img(g[a:b]) if g is not None else None,
               xp=img(x[a - 1:a]) if (a > 0 and geo.z_active and drop_halo != "prev") else None,
               xn=img(x[b:b + 1]) if (b < nzg and geo.z_active and drop_halo != "next") else None)
    ws = geo.workspace()
    ws.fill_(WS_FILL)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None}, ws=ws)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    head = (geo.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]))
    tail = (float(sigma), float(lam), out.data_ptr(), nv.ptr(ws), nv.current_stream(geo.device))
    if g is None:
        nv.check(nv.lib().tv_cp_dual(*head, *tail))
    else:
        nv.check(nv.lib().tv_cp_dual_wtv(*head, nv.ptr(dev["gw"]), *tail))
    return dev["q"].cpu().numpy(), float(out.item())


def gpu_gap(x, q, x0, g, lam, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None):
    """tv_dual_gap_wtv on local planes [a, b), halo planes of x and q passed by hand; returns the three scalars"""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    geo = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(geo)
    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]), x0=img(x0[a:b]), gw=img(g[a:b]),
               xp=img(x[a - 1:a]) if (a > 0 and geo.z_active) else None, xn=img(x[b:b + 1]) if (b < nzg and geo.z_active) else None,
               qp=img(q[a - 1:a, cb]) if (a > 0 and geo.z_active) else None, qn=img(q[b:b + 1, cf]) if (b < nzg and geo.z_active) else None)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None})
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_dual_gap_wtv(geo.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), nv.ptr(dev["qp"]),
                                      nv.ptr(dev["qn"]), nv.ptr(dev["x0"]), nv.ptr(dev["gw"]), float(lam), out.data_ptr(),
                                      nv.ptr(geo.workspace()), nv.current_stream(geo.device)))
    return tuple(out.cpu().tolist())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


GAP_INPUTS = ("x", "q", "x0", "gw", "xp", "xn", "qp", "qn")


# ------------------------------------------------------------------------------------------------
# 1. tv_cp_dual_wtv: parity against the restatement, and the projection invariants
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_dual_entry_point_matches_the_restatement(shape, scheme, dtype):
    """every weighting, natural and explicit pitch.  Invariants: |q|_2 <= r (1 + RTOL) at every site; where the restatement has
    |v| < r (1 - 10 RTOL) the new q is the GPU's own v BIT FOR BIT (v from a second call with g scaled by 1e6: every g > 0 site is then
    inside its ball); q == 0 at every g = 0 site; no NaN"""
    rtol = RTOL[dtype]
    for weighting in WEIGHTINGS:
        x, q, _, g, kw = kernel_inputs(shape, scheme, dtype, weighting)
        wq, wwtv, v, nv_, r = ref_dual(x, q, g, SIGMA, LAM, scheme, kw)
        pos = r > 0.0
        shares = (float(np.mean(nv_[pos] <= r[pos])), float(np.mean(nv_[pos] > r[pos])))
        assert min(shares) >= 0.1, shares                               # a condition on the inputs: both sides of |v| = r
        assert 0.25 <= float(np.mean(~pos)) <= 0.42
        tol = rtol * float(np.max(np.abs(wq)))
        inside = np.broadcast_to((pos & (nv_ < r * (1.0 - 10.0 * rtol)))[:, None], v.shape)
        zero = np.broadcast_to((~pos)[:, None], v.shape)
        assert float(np.max(nv_[pos] / (1e6 * r[pos]))) < 1.0
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            what = "%s %s pitch %r" % (weighting, scheme, pitch)
            keep = {}
            gq, wtv = gpu_dual(x, q, g, SIGMA, LAM, scheme, dtype, kw, pitch=pitch, keep=keep)
            gv, _ = gpu_dual(x, q, (1e6 * g.astype(np.float64)).astype(dtype), SIGMA, LAM, scheme, dtype, kw, pitch=pitch)
            gn = np.sqrt(np.sum(gq.astype(np.float64) ** 2, axis=1))
            print("%s: max|dq| %.3e (tol %.3e)  |d wtv| %.3e (tol %.3e)  max(|q| / r) - 1 %.3e  shares %.2f %.2f" % (
                what, np.max(np.abs(gq - wq)), tol, abs(wtv - wwtv), rtol * wwtv, np.max(gn[pos] / r[pos]) - 1.0, *shares))
            assert gq.dtype == dtype and not np.isnan(gq).any() and np.isfinite(gq).all()
            assert float(np.max(np.abs(gq - wq))) <= tol, what
            assert abs(wtv - wwtv) <= rtol * wwtv, what                 # (every term of the sum is >= 0)
            assert bool(np.all(gn <= r * (1.0 + rtol))), what
            assert float(np.max(np.abs(gv - v)[np.broadcast_to(pos[:, None], v.shape)])) <= rtol * float(np.max(np.abs(v))), what
            np.testing.assert_array_equal(_bits(gq)[inside], _bits(gv)[inside], err_msg=what)
            assert not gq[zero].any(), what
            _untouched(keep, ("x", "xp", "xn", "gw"))
            _ws_beyond_the_partials_untouched(keep["ws"])
            if pitch != (0, 0):
                _pads_are_zero(keep["dev"]["q"])


# ------------------------------------------------------------------------------------------------
# 2. constant g is tv_cp_dual with another lambda
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("c", (1.0, 0.5))
def test_constant_g_equals_the_plain_dual_step(c, scheme, dtype):
    shape, rtol = (3, 2, 16, 20), RTOL[dtype]
    x, q, _, _, kw = kernel_inputs(shape, scheme, dtype, "plain")
    g = np.full(shape, c, dtype=dtype)
    got = gpu_dual(x, q, g, SIGMA, LAM, scheme, dtype, kw)
    plain = gpu_dual(x, q, None, SIGMA, LAM * c, scheme, dtype, kw)
    print("c %g %s %s: max|dq| %.3e  scalars %.12e %.12e" % (c, scheme, np.dtype(dtype).name, np.max(np.abs(got[0] - plain[0])), got[1], plain[1]))
    assert float(np.max(np.abs(got[0] - plain[0]))) <= rtol * float(np.max(np.abs(plain[0])))
    assert abs(got[1] - c * plain[1]) <= rtol * c * plain[1]            # c |D x|_{2,1}


# ------------------------------------------------------------------------------------------------
# 3. z-ranges: planes [a, b) with hand-passed halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
Z_SHAPE = (5, 2, 16, 20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_z_ranges_equal_the_whole_volume(scheme, dtype):
    x, q, _, g, kw = kernel_inputs(Z_SHAPE, scheme, dtype, "plain")
    wq, wwtv = gpu_dual(x, q, g, SIGMA, LAM, scheme, dtype, kw)
    Dx = orc.D(x.astype(np.float64), scheme, **kw)
    gn = g.astype(np.float64) * np.sqrt(np.sum(Dx * Dx, axis=1))
    parts = {}
    for a, b in ((0, 2), (2, 5), (1, 4)):
        keep = {}
        gq, wtv = gpu_dual(x, q, g, SIGMA, LAM, scheme, dtype, kw, z_range=(a, b), keep=keep)
        np.testing.assert_array_equal(gq, wq[a:b], err_msg="planes [%d, %d)" % (a, b))
        _untouched(keep, ("x", "xp", "xn", "gw"))
        want = float(np.sum(gn[a:b]))                                   # the restatement's share of those planes
        assert abs(wtv - want) <= RTOL[dtype] * want, (a, b)
        parts[(a, b)] = wtv
    print("%s %s: parts %.17g + %.17g whole %.17g" % (scheme, np.dtype(dtype).name, parts[(0, 2)], parts[(2, 5)], wwtv))
    assert abs(parts[(0, 2)] + parts[(2, 5)] - wwtv) <= RTOL[dtype] * wwtv


@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    x, q, _, g, kw = kernel_inputs(Z_SHAPE, scheme, np.float32, "plain")
    # a forward difference reads the next slab, a backward one the previous (central, hybrid: both)
    sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))
    for side in sides:
        keep = {}
        with pytest.raises(ValueError, match=r"x_%s.*halo.*code -2" % side):
            gpu_dual(x, q, g, SIGMA, LAM, scheme, np.float32, kw, z_range=(1, 4), keep=keep, drop_halo=side)
        torch.cuda.synchronize()
        _untouched(keep, ("x", "q", "gw", "xp", "xn"))
        assert bool((keep["ws"] == WS_FILL).all())


# ------------------------------------------------------------------------------------------------
# 4. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_marching_form_equals_one_site_form(scheme, tvopt):
    """arrays to 1e-5 max|.|, the scalar to 1e-5 (tests/test_gpu_cp_huber.py).  g has a stripe of zeros that crosses tile and lane boundaries:
    columns 250 - 262 and rows 5 - 11.  sigma = 0.3 here: an entry of a site inside its ball whose difference is zero by the boundary rule (a
    quarter of the entries with two planes and two frames) keeps its q, so for 90 % of the entries to change less than 40 % of the sites may
    lie inside -- with sigma = 0.3 that share is 0.19 - 0.47 of the g > 0 sites over the four schemes (fp64 restatement, same distributions)"""
    shape, dtype, sigma = (2, 2, 1024, 1024), np.float32, 0.3
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, shape[0], shape[1], **PLAIN_KW)
    x = 60.0 * rng.random(shape, dtype=np.float32)
    q = LAM * (rng.random((shape[0], nd) + shape[1:], dtype=np.float32) - 0.5)
    g = make_g(shape, dtype)
    g[..., :, 250:263] = 0.0
    g[..., 5:12, :] = 0.0
    march = gpu_dual(x, q, g, sigma, LAM, scheme, dtype, PLAIN_KW)
    tvopt("TV_NO_MARCH", 1)
    site = gpu_dual(x, q, g, sigma, LAM, scheme, dtype, PLAIN_KW)
    tol = 1e-5 * float(np.max(np.abs(site[0])))
    moved = float(np.mean(site[0] != q))
    print("%s: max|dq| %.3e (tol %.3e)  wtv %.9e / %.9e  entries changed %.3f" % (scheme, np.max(np.abs(march[0] - site[0])), tol, march[1], site[1],
                                                                              moved))
    assert float(np.max(np.abs(march[0] - site[0]))) <= tol
    assert abs(march[1] - site[1]) <= 1e-5 * site[1]
    assert np.isfinite(march[1]) and march[1] > 0.0 and moved > 0.9
    zero = np.broadcast_to((g == 0.0)[:, None], q.shape)
    assert not march[0][zero].any() and not site[0][zero].any()


@pytest.mark.parametrize("scheme,m,marches", [("central", 8, True), ("upwind", 16, True), ("downwind", 16, False)])
def test_dual_marching_rule_at_8_and_16_frames(scheme, m, marches, tvopt):
    """one plane of m frames, fp32: (central, 8) is the marching instantiation with the most registers, (upwind, 16) the only 16-frame one that
    exists, (downwind, 16) is kept off the marching path by the exclusion rule (csrc/tv_host.h, wtv_spill16) and must run the one-site kernel
    -- bit-equal to the TV_NO_MARCH call, not an error.  Tolerances of the test above."""
    shape, dtype, sigma = (1, m, 1024, 1024), np.float32, 0.3
    rng = np.random.default_rng(12)
    nd = orc.num_channels(scheme, shape[0], shape[1], **PLAIN_KW)
    x = 60.0 * rng.random(shape, dtype=np.float32)
    q = LAM * (rng.random((shape[0], nd) + shape[1:], dtype=np.float32) - 0.5)
    g = make_g(shape, dtype)
    dflt = gpu_dual(x, q, g, sigma, LAM, scheme, dtype, PLAIN_KW)
    tvopt("TV_NO_MARCH", 1)
    site = gpu_dual(x, q, g, sigma, LAM, scheme, dtype, PLAIN_KW)
    tol = 1e-5 * float(np.max(np.abs(site[0])))
    same = bool(np.array_equal(dflt[0], site[0]))
    print("%s M = %d: max|dq| %.3e (tol %.3e)  wtv %.9e / %.9e  bit-equal %r" % (scheme, m, np.max(np.abs(dflt[0] - site[0])), tol, dflt[1], site[1], same))
    assert float(np.max(np.abs(dflt[0] - site[0]))) <= tol
    assert abs(dflt[1] - site[1]) <= 1e-5 * site[1] and np.isfinite(dflt[1]) and dflt[1] > 0.0
    if not marches:
        assert same and dflt[1] == site[1]
    assert not dflt[0][np.broadcast_to((g == 0.0)[:, None], q.shape)].any()


# ------------------------------------------------------------------------------------------------
# 5. tv_dual_gap_wtv
# ------------------------------------------------------------------------------------------------
def _check_gap(got, ref, dtype, what, lam=LAM):
    rtol, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    wtv, fid, gap, terms = ref
    print("%s got %r ref %r  |d gap| %.3e (tol %.3e)" % (what, tuple(got), ref[:3], abs(got[2] - gap), rtol * terms))
    assert abs(got[0] - wtv) <= rtol * wtv, what
    assert abs(got[1] - fid) <= rtol * fid, what
    assert abs(got[2] - gap) <= rtol * terms, what
    assert got[2] >= -16.0 * eps * (fid + lam * wtv), what              # a feasible q: the gap is >= 0 up to the fp floor


@functools.lru_cache(maxsize=None)
def feasible_q(shape, scheme, dtype, weighting):
    """the output of the dual step's restatement (test 1), rounded to the dtype: |q|_2 <= LAM g per site"""
    x, q, _, g, kw = kernel_inputs(shape, scheme, dtype, weighting)
    fq = ref_dual(x, q, g, SIGMA, LAM, scheme, kw)[0].astype(dtype)
    fq.setflags(write=False)
    return fq


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_gap_matches_the_restatement_and_writes_nothing(shape, scheme, dtype):
    for weighting in WEIGHTINGS:
        x, _, x0, g, kw = kernel_inputs(shape, scheme, dtype, weighting)
        q = feasible_q(shape, scheme, dtype, weighting)
        ref = ref_gap(x, q, x0, g, LAM, scheme, kw)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            keep = {}
            got = gpu_gap(x, q, x0, g, LAM, scheme, dtype, kw, pitch=pitch, keep=keep)
            _check_gap(got, ref, dtype, "%s %s pitch %r" % (weighting, scheme, pitch))
            _untouched(keep, GAP_INPUTS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_gap_z_range_partials_add_up(scheme, dtype):
    x, _, x0, g, kw = kernel_inputs(Z_SHAPE, scheme, dtype, "plain")
    q = feasible_q(Z_SHAPE, scheme, dtype, "plain")
    ref = ref_gap(x, q, x0, g, LAM, scheme, kw)
    whole = gpu_gap(x, q, x0, g, LAM, scheme, dtype, kw)
    _check_gap(whole, ref, dtype, "whole")
    for cut in ((0, 2, 5), (0, 1, 4, 5)):
        parts = np.zeros(3)
        for a, b in zip(cut[:-1], cut[1:]):
            keep = {}
            parts += np.array(gpu_gap(x, q, x0, g, LAM, scheme, dtype, kw, z_range=(a, b), keep=keep))
            _untouched(keep, GAP_INPUTS)
        print("%s %s cut %r: parts %r whole %r" % (scheme, np.dtype(dtype).name, cut, tuple(parts), whole))
        for k, scale in enumerate((ref[0], ref[1], ref[3])):
            assert abs(parts[k] - whole[k]) <= RTOL[dtype] * scale, (cut, k)


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 2) with the per-site radius, and of its duality gap
# ------------------------------------------------------------------------------------------------
REG = 10.0


def np_adaptive(x0, n_iter, lam, g, scheme, kw, gamma=1.0, state=None):
    """n_iter iterations from ``state`` = (x, x_bar, q, tau, sigma) (default: the start); returns (x, loss, state)"""
    x0, g = np.asarray(x0, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if state is None:
        L2 = orc.normal_spectral_bound(scheme, x0.shape, **kw)
        state = (x0.copy(), x0.copy(), np.zeros_like(orc.D(x0, scheme, **kw)), 1.0 / np.sqrt(L2), 1.0 / np.sqrt(L2))
    x, xb, q, tau, sigma = state
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project_r(q + sigma * Dxb, lam * g)
        xn = (x - tau * orc.D_T(q, scheme, **kw) + tau * x0) / (1.0 + tau)
        theta = 1.0 / np.sqrt(1.0 + 2.0 * gamma * tau)
        xb = xn + theta * (xn - x)
        x = xn
        loss[k] = 0.5 * np.sum((x - x0) ** 2) + lam * np.sum(g * np.sqrt(np.sum(Dxb * Dxb, axis=1)))
        tau, sigma = theta * tau, sigma / theta
    return x, loss, (x, xb, q, tau, sigma)


def np_run_until(x0, rel_gap, max_iter, check_every, lam, g, scheme, kw):
    """the iteration count of ``run_until`` in the restatement, and its last (primal, gap)"""
    state, done = None, 0
    while True:
        _, _, state = np_adaptive(x0, check_every, lam, g, scheme, kw, state=state)
        done += check_every
        wtv, fid, gap, _ = ref_gap(state[0], state[2], x0, g, lam, scheme, kw)
        if gap <= rel_gap * (fid + lam * wtv) or done >= max_iter:
            return done, fid + lam * wtv, gap


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, n_iter, f32_input=False):
    x0, g = noisy_square(shape), make_g(shape, np.float64)
    if f32_input:
        x0, g = x0.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
    return np_adaptive(x0, n_iter, REG, g, scheme, _kw_of(shape))


def _solver(pytv, shape, dtype, scheme, g=None, reg=REG, **how):
    g = make_g(shape, dtype) if g is None else g
    return pytv.solvers.AdaptiveTVChambollePock(torch.as_tensor(noisy_square(shape).astype(dtype)).cuda(), reg, torch.as_tensor(g).cuda(),
                                                scheme=scheme, **_kw_of(shape), **how)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
def test_gap_of_a_restated_pair_after_300_iterations(scheme, dtype):
    """(x, q) of 300 restatement iterations, rounded to the dtype: the three scalars within the scalar tolerance, the gap above the floor"""
    shape = (3, 2, 16, 20)
    x0, g, kw = noisy_square(shape), make_g(shape, np.float64), _kw_of(shape)
    if dtype == np.float32:
        x0, g = x0.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
    _, _, state = np_adaptive(x0, 300, REG, g, scheme, kw)
    x, q = state[0].astype(dtype), state[2].astype(dtype)
    ref = ref_gap(x, q, x0, g, REG, scheme, kw)
    got = gpu_gap(x, q, x0.astype(dtype), g.astype(dtype), REG, scheme, dtype, kw)
    _check_gap(got, ref, dtype, "%s %s after 300 iterations: relative gap %.3e" % (scheme, np.dtype(dtype).name, ref[2] / (ref[1] + REG * ref[0])),
               lam=REG)


# ------------------------------------------------------------------------------------------------
# 6. solver
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme):
    import pytv
    wx, wloss, _ = np_trajectory(shape, scheme, 30)
    cp = _solver(pytv, shape, np.float64, scheme)
    assert cp.it == 0 and cp.gamma == 1.0 and cp.fused is False and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape))
    with pytest.raises(ValueError, match="one-sweep"):
        cp.set_fused(True)
    loss = cp.run(30)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(noisy_square(shape))))
    assert cp.it == 30 and cp.fused is False
    # run(10); run(20) is run(30) bit for bit: the schedule continues
    two = _solver(pytv, shape, np.float64, scheme)
    np.testing.assert_array_equal(np.concatenate([two.run(10), two.run(20)]), loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.x_bar, cp.x_bar) and torch.equal(two.q, cp.q)
    # reset() restarts the schedule: the first run again, bit for bit
    two.reset()
    assert two.it == 0 and torch.equal(two.x, two.x0) and torch.equal(two.x_bar, two.x0) and not bool(two.q.any())
    np.testing.assert_array_equal(two.run(30), loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.q, cp.q)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme):
    """the fp32 tolerance of tests/test_gpu_cp_huber.py against the fp64 restatement on the fp32-rounded input: loss rtol 1e-5; result rtol
    1e-5, atol 2e-3"""
    import pytv
    wx, wloss, _ = np_trajectory(shape, scheme, 30, f32_input=True)
    cp = _solver(pytv, shape, np.float32, scheme)
    loss = cp.run(30)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("c", (1.0, 0.5))
def test_constant_g_reproduces_the_accelerated_solver(c, scheme):
    """g = c everywhere is plain TV with the weight REG c: the kernel pair of ``AcceleratedChambollePock`` on the GPU, to the fp64 trajectory
    tolerance (the two dual epilogues round differently: v / max(1, n / lam) against v (r / n))"""
    import pytv
    shape = (3, 2, 16, 20)
    cp = _solver(pytv, shape, np.float64, scheme, g=np.full(shape, c))
    acc = pytv.solvers.AcceleratedChambollePock(torch.as_tensor(noisy_square(shape).copy()).cuda(), REG * c, scheme=scheme, **_kw_of(shape))
    acc.set_fused(False)
    loss, wloss = cp.run(30), acc.run(30)
    dx = float(torch.max(torch.abs(cp.result() - acc.result())))
    print("c %g %s: loss rel %.3e  max|dx| %.3e" % (c, scheme, np.max(np.abs(loss / wloss - 1.0)), dx))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert dx <= 1e-9 * float(np.max(np.abs(noisy_square(shape))))
    np.testing.assert_allclose(cp.duality_gap(), acc.duality_gap(), rtol=1e-9)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", STOP_SHAPES)
def test_run_until_certifies_where_the_restatement_does(shape, scheme):
    import pytv
    kw, g = _kw_of(shape), make_g(shape, np.float64)
    want, wprimal, wgap = np_run_until(noisy_square(shape), 1e-4, 600, 10, REG, g, scheme, kw)
    assert want < 600
    cp = _solver(pytv, shape, np.float64, scheme)
    loss, info = cp.run_until(1e-4, 600, 10)
    print("%s %s: %r  restated: %d iterations, primal %.12e gap %.3e" % (scheme, shape, info, want, wprimal, wgap))
    assert info["converged"] is True and abs(info["iterations"] - want) <= 10 and len(loss) == info["iterations"] == cp.it
    assert 0.0 <= info["gap"] <= 1e-4 * info["primal"] and info["dual"] == info["primal"] - info["gap"]
    assert info["error_bound"] == np.sqrt(2 * info["gap"])
    if info["iterations"] == want:
        np.testing.assert_allclose(info["primal"], wprimal, rtol=1e-10)
        assert abs(info["gap"] - wgap) <= 1e-10 * wprimal
    # the certificate leaves the state of the loop alone
    state = [t.clone() for t in (cp.x, cp.x_bar, cp.q, cp.g)]
    assert cp.duality_gap() == (info["primal"], info["dual"], info["gap"])
    assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q, cp.g)))


def test_constructor_refuses_bad_weights_and_regularization():
    import pytv
    shape = (1, 1, 24, 28)
    x0 = torch.as_tensor(noisy_square(shape).copy()).cuda()
    for bad in (-1e-3, float("nan"), float("inf"), float("-inf")):
        g = np.ones(shape)
        g[0, 0, 3, 4] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            pytv.solvers.AdaptiveTVChambollePock(x0, REG, g)
    for g in (np.ones((1, 1, 24, 27)), np.ones((24, 28)), np.ones(shape, dtype=np.int64)):
        with pytest.raises(ValueError, match="shape"):
            pytv.solvers.AdaptiveTVChambollePock(x0, REG, g)
    for reg in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="regularization"):
            pytv.solvers.AdaptiveTVChambollePock(x0, reg, np.ones(shape))
    # all-zero g is allowed: nothing regularises, the solver returns x0
    cp = pytv.solvers.AdaptiveTVChambollePock(x0, REG, np.zeros(shape), scheme="upwind")
    cp.run(5)
    assert not bool(cp.q.any())
    assert float(torch.max(torch.abs(cp.result() - x0))) <= 8 * np.finfo(np.float64).eps * float(torch.max(torch.abs(x0)))
    bools = pytv.solvers.AdaptiveTVChambollePock(x0, REG, np.ones(shape, dtype=bool), scheme="upwind")
    assert bools.g.dtype == x0.dtype and bool((bools.g == 1).all())


# ------------------------------------------------------------------------------------------------
# 7. a protected region is left alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(1, 1, 32, 40), (5, 5, 16, 20)])
def test_protected_region_is_left_alone(shape, scheme, dtype):
    """g = 0 on a block, 1 elsewhere.  Every site of the block keeps q = 0 exactly, so D^T q = 0 at the voxels whose neighbouring sites all lie
    in the block -- the block eroded by one site along every active axis -- and there x <- (x + tau x0) / (1 + tau) stays at x0 to rounding:
    max|x - x0| <= 8 eps max|x0| after 50 iterations.  Outside the block the image is smoothed: RMS(x - x0) > 10 times that bound."""
    import pytv
    nz, m, ny, nx = shape
    block = [slice(1, 4) if n > 1 else slice(0, 1) for n in (nz, m)] + [slice(ny // 4, ny - ny // 4), slice(nx // 4, nx - nx // 4)]
    eroded = [slice(s.start + 1, s.stop - 1) if n > 1 else s for s, n in zip(block, shape)]
    g = np.ones(shape, dtype=dtype)
    g[tuple(block)] = 0.0
    cp = _solver(pytv, shape, dtype, scheme, g=g)
    cp.run(50)
    x, x0, q = cp.result().cpu().numpy().astype(np.float64), cp.x0.cpu().numpy().astype(np.float64), cp.q.cpu().numpy()
    bound = 8.0 * float(np.finfo(dtype).eps) * float(np.max(np.abs(x0)))
    inside = float(np.max(np.abs(x - x0)[tuple(eroded)]))
    out_mask = g > 0
    rms = float(np.sqrt(np.mean(((x - x0) ** 2)[out_mask])))
    print("%s %s %s: max|x - x0| in the eroded block %.3e (bound %.3e), RMS outside %.3e" % (scheme, shape, np.dtype(dtype).name, inside, bound, rms))
    assert x[tuple(eroded)].size > 0
    assert not q[(block[0], slice(None)) + tuple(block[1:])].any()       # all contributing q are 0
    assert inside <= bound
    assert rms > 10.0 * bound


# ------------------------------------------------------------------------------------------------
# 8. front-end and helper
# ------------------------------------------------------------------------------------------------
def np_edge_weights(img, kappa, scheme="upwind"):
    vol = np.asarray(img, dtype=np.float64)
    vol = vol.reshape((1, 1) + vol.shape) if vol.ndim == 2 else vol.reshape(vol.shape[0], 1, *vol.shape[1:])
    Dx = orc.D(vol, scheme, reg_z_over_reg=1.0)
    n = np.sqrt(np.sum(Dx * Dx, axis=1))
    return (1.0 / (1.0 + (n / kappa) ** 2)).reshape(np.shape(img))


def test_denoise_tv_adaptive_front_end():
    import pytv
    shape = (1, 1, 24, 28)
    img = noisy_square(shape)[0, 0].astype(np.float32)
    g2 = make_g(shape, np.float32)[0, 0]
    vol = torch.as_tensor(img.reshape(shape)).cuda()
    out = pytv.denoise_tv_adaptive(img, 10.0, g2, rel_gap=1e-3, max_num_iter=400)
    ref = pytv.solvers.AdaptiveTVChambollePock(vol, 10.0, torch.as_tensor(g2.reshape(shape)).cuda(), scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-3, 400, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] % 10 == 0 and info["iterations"] < 400
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == img.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # 3-D input, never converges: exactly 40 iterations, the solver's run(40)
    stack = np.stack([img, img[::-1], img])
    g3 = make_g((3, 1, 24, 28), np.float32)[:, 0]
    out = pytv.denoise_tv_adaptive(stack, 10.0, g3, rel_gap=-1.0, max_num_iter=40, scheme="hybrid", check_every=20)
    ref = pytv.solvers.AdaptiveTVChambollePock(torch.as_tensor(stack.reshape(3, 1, 24, 28).copy()).cuda(), 10.0,
                                               torch.as_tensor(g3.reshape(3, 1, 24, 28).copy()).cuda(), scheme="hybrid", reg_z_over_reg=1.0)
    ref.run(40)
    assert out.shape == stack.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(stack.shape))
    # reg_weights=None is all ones; torch in -> device tensor out; 4-D and a wrong shape refused
    ones = pytv.denoise_tv_adaptive(img, 10.0, None, max_num_iter=30, rel_gap=-1.0)
    np.testing.assert_array_equal(ones, pytv.denoise_tv_adaptive(img, 10.0, np.ones_like(img), max_num_iter=30, rel_gap=-1.0))
    t = pytv.denoise_tv_adaptive(vol[0, 0], 10.0, g2, max_num_iter=30)
    assert isinstance(t, torch.Tensor) and t.is_cuda and torch.equal(t.cpu(), torch.as_tensor(pytv.denoise_tv_adaptive(img, 10.0, g2, max_num_iter=30)))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.denoise_tv_adaptive(np.zeros((1, 1, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        pytv.denoise_tv_adaptive(img, 10.0, g2[:-1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_edge_stopping_weights_match_the_restatement(scheme, dtype):
    import pytv
    for shape in ((24, 28), (3, 16, 20)):
        img = (0.1 * noisy_square((1, 1) + shape if len(shape) == 2 else (shape[0], 1) + shape[1:])).reshape(shape).astype(dtype)
        want = np_edge_weights(img, 1.5, scheme)
        got = pytv.edge_stopping_weights(img, 1.5, scheme=scheme)
        print("%s %s %r: max|dg| %.3e  min g %.3e" % (scheme, np.dtype(dtype).name, shape, np.max(np.abs(got - want)), got.min()))
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == img.shape
        assert float(np.max(np.abs(got - want))) <= RTOL[dtype] * 1.0                                # max|g| = 1
        assert got.min() > 0.0 and got.max() <= 1.0 and want.min() < 0.1 and want.max() > 0.5
    t = pytv.edge_stopping_weights(torch.as_tensor(img).cuda(), 1.5, scheme=scheme)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), got)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.edge_stopping_weights(np.zeros((1, 1, 8, 8)), 1.0)


STEP_SHAPE, STEP_HEIGHT, STEP_WEIGHT, STEP_KAPPA = (24, 28), 8.0, 10.0, 3.0


@functools.lru_cache(maxsize=None)
def noisy_step():
    """a vertical edge of low contrast -- 8 grey levels, left half 0 -- plus N(0, 1) noise"""
    ny, nx = STEP_SHAPE
    img = np.zeros(STEP_SHAPE)
    img[:, nx // 2:] = STEP_HEIGHT
    return img + np.random.default_rng(3).standard_normal(STEP_SHAPE)


def edge_jump(u):
    """mean difference of the two columns next to the edge"""
    nx = STEP_SHAPE[1]
    return float(np.mean(u[:, nx // 2] - u[:, nx // 2 - 1]))


def test_edge_stopping_weights_keep_a_low_contrast_edge():
    """the restatement first (CPU, 400 iterations of the loop above, upwind): the jump across the edge is larger with g = edge-stopping weights
    of the noisy input than with g = 1 at the same weight; then the same ordering on the GPU.  No fixed number is asserted."""
    import pytv
    noisy = noisy_step()
    vol = noisy.reshape((1, 1) + STEP_SHAPE)
    g = np_edge_weights(noisy, STEP_KAPPA)
    kw = dict(reg_z_over_reg=1.0)
    w_edge = np_adaptive(vol, 400, STEP_WEIGHT, g.reshape(vol.shape), "upwind", kw)[0][0, 0]
    w_flat = np_adaptive(vol, 400, STEP_WEIGHT, np.ones(vol.shape), "upwind", kw)[0][0, 0]
    assert edge_jump(w_edge) > edge_jump(w_flat)                        # the ordering the restatement shows
    g_gpu = pytv.edge_stopping_weights(noisy, STEP_KAPPA)
    edge = pytv.denoise_tv_adaptive(noisy, STEP_WEIGHT, g_gpu, rel_gap=1e-8, max_num_iter=400)
    flat = pytv.denoise_tv_adaptive(noisy, STEP_WEIGHT, None, rel_gap=1e-8, max_num_iter=400)
    print("jump across the edge (clean: %g): edge-stopping weights %.4f (restated %.4f), uniform %.4f (restated %.4f); noisy %.4f" % (
        STEP_HEIGHT, edge_jump(edge), edge_jump(w_edge), edge_jump(flat), edge_jump(w_flat), edge_jump(noisy)))
    assert edge.dtype == np.float64 and edge_jump(edge) > edge_jump(flat)
