"""The one-site kernels of the adaptive Huber-TV solver on the GPU (``-m gpu``): tv_cp_dual_hwtv and tv_dual_gap_hwtv through the C-ABI against
NumPy float64 over ``orc.D`` / ``orc.D_T`` -- four schemes, four weightings, pitched and unpitched arrays, scalar rows and 16-byte lanes,
hand-made slabs with halo planes --, the exactness statements on bits, a degenerate alpha against tv_cp_dual_wtv bit for bit, and g = 1
against tv_cp_dual_huber / tv_dual_gap_huber / ``HuberChambollePock``.

Inputs, scalars (SIGMA, LAM, ALPHA = 2), the weight g and the conditions on the inputs are those of tests/test_gpu_cp_hwtv_sweep.py (its
``problem``, which asserts the 2 % shares while it builds the float64 reference), on that module's vector shape 7x3x10x64 and on two shapes
whose rows are no whole 16-byte lanes in fp32 or whose planes are single: 3x2x16x20 and 1x1x32x40.
Tolerances: arrays to RTOL = 1e-5 (fp32) / 1e-11 (fp64) of the array's max; scalars to the same RTOL of the reference sum (the gap: of the sum
of the absolute values of its terms, as tests/test_gpu_cp_huber.py bounds its own); fp64 trajectories: loss rtol 1e-10, result 1e-9 max|x0|."""
import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_accel_sweep import E_HALO, LAM, RTOL, SIGMA, WEIGHTINGS, _explicit_pitch, _geom, _pads_are_zero, _storage, z_channels
from test_gpu_cp_huber import REG, noisy_square
from test_gpu_cp_hwtv_sweep import ALPHA, ALPHA_DEGENERATE, np_gap_hwtv, problem

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 16, 20), (1, 1, 32, 40), (7, 3, 10, 64)]
DTYPES = [np.float64, np.float32]
WS_FILL = -7.0


@pytest.fixture(scope="module")
def nvlib():
    import pytv  # noqa: F401
    from pytv import _native as nv
    return nv


def _up(g, arr, grad=False):
    t = (g.new_grad if grad else g.new_image)(arr.shape[0])
    t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
    return t


def _plane(g, arr):
    """one plane of an image-like array (a halo plane), in the geometry's layout"""
    return _up(g, arr[None])


def gpu_dual(nv, P, x, q, gw, alpha=ALPHA, pitch=(0, 0), z_range=None, drop=None, entry="hwtv"):
    """tv_cp_dual_hwtv (or, entry = "wtv" / "huber", the sibling on the same arrays) on the planes [a, b) with hand-passed halo planes of x.
    Returns (status, q after the call, the scalar, keep): keep has the device arrays, copies of their storage before the call and the workspace."""
    nzg = P.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = _geom(nv, P, pitch, a, b)
    dev = dict(x=_up(g, x[a:b]), q=_up(g, q[a:b], True), gw=_up(g, gw[a:b]),
               xp=_plane(g, x[a - 1]) if (a > 0 and g.z_active and drop != "prev") else None,
               xn=_plane(g, x[b]) if (b < nzg and g.z_active and drop != "next") else None)
    ws = g.workspace()
    ws.fill_(WS_FILL)
    keep = dict(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None}, ws=ws)
    out = torch.full((1,), 123.0, dtype=torch.float64, device="cuda")
    ptr, st = nv.ptr, nv.current_stream(g.device)
    head = (g.ref, ptr(dev["x"]), ptr(dev["xp"]), ptr(dev["xn"]), ptr(dev["q"]))
    if entry == "hwtv":
        rc = nv.lib().tv_cp_dual_hwtv(*head, ptr(dev["gw"]), SIGMA, LAM, alpha, out.data_ptr(), ptr(ws), st)
    elif entry == "wtv":
        rc = nv.lib().tv_cp_dual_wtv(*head, ptr(dev["gw"]), SIGMA, LAM, out.data_ptr(), ptr(ws), st)
    else:
        rc = nv.lib().tv_cp_dual_huber(*head, SIGMA, LAM, alpha, out.data_ptr(), ptr(ws), st)
    torch.cuda.synchronize()
    return rc, dev["q"], float(out.item()), keep


def gpu_gap(nv, P, x, q, x0, gw, pitch=(0, 0), z_range=None, entry="hwtv"):
    nzg = P.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = _geom(nv, P, pitch, a, b)
    cb, cf = z_channels(P.scheme)
    lo, hi = (a > 0 and g.z_active), (b < nzg and g.z_active)
    dev = dict(x=_up(g, x[a:b]), q=_up(g, q[a:b], True), x0=_up(g, x0[a:b]), gw=_up(g, gw[a:b]),
               xp=_plane(g, x[a - 1]) if lo else None, xn=_plane(g, x[b]) if hi else None,
               qp=_plane(g, q[a - 1, cb]) if lo else None, qn=_plane(g, q[b, cf]) if hi else None)
    before = {k: _storage(v).clone() for k, v in dev.items() if v is not None}
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    ptr, st = nv.ptr, nv.current_stream(g.device)
    head = (g.ref, ptr(dev["x"]), ptr(dev["xp"]), ptr(dev["xn"]), ptr(dev["q"]), ptr(dev["qp"]), ptr(dev["qn"]), ptr(dev["x0"]))
    if entry == "hwtv":
        nv.check(nv.lib().tv_dual_gap_hwtv(*head, ptr(dev["gw"]), LAM, ALPHA, out.data_ptr(), ptr(g.workspace()), st))
    else:
        nv.check(nv.lib().tv_dual_gap_huber(*head, LAM, ALPHA, out.data_ptr(), ptr(g.workspace()), st))
    got = tuple(out.cpu().tolist())
    for k, v in before.items():
        assert torch.equal(_storage(dev[k]), v), (k, "input written to")        # reduce-only
    return got


def _untouched(keep, names):
    for k in names:
        if keep["dev"][k] is not None:
            assert torch.equal(_storage(keep["dev"][k]), keep["before"][k]), k


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------------
# 1. one dual step against NumPy, and the exactness statements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_dual_step_matches_numpy_and_is_exact_where_it_says(nvlib, shape, scheme, dtype):
    """q and the scalar against the float64 reference.  On bits: g = 0 sites end with q == 0 in every channel; a site inside its ball stores
    v = shrink (q + sigma D x_bar) unchanged -- v is taken from the SAME kernel, run with lambda g large enough that no site projects (the
    shrink factor r / (r + sigma alpha) depends on r, so that run scales alpha with it: r' = K r, alpha' = K alpha gives the same factor up to
    the rounding of K r, and K a power of two makes it the same bits); |q|_2 <= r (1 + 4 eps) everywhere; inputs untouched, pads zero."""
    nv = nvlib
    rt, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    for weighting in WEIGHTINGS:
        P = problem(scheme, shape, dtype, weighting)
        tol = rt * float(np.max(np.abs(P.qn)))
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            what = "%s %s %s %s pitch %r" % (scheme, shape, np.dtype(dtype).name, weighting, pitch)
            rc, q, hwtv, keep = gpu_dual(nv, P, P.xbar, P.q, P.g, pitch=pitch)
            assert rc == 0, (what, nv.lib().tv_last_error())
            gq = q.cpu().numpy()
            err = float(np.max(np.abs(gq - P.qn)))
            print("%s: max|dq| %.3e (tol %.3e) hwtv %.12e (ref %.12e) shares %r" % (what, err, tol, hwtv, P.hub, P.shares))
            assert gq.dtype == dtype and np.isfinite(gq).all() and err <= tol, (what, err, tol)
            assert abs(hwtv - P.hub) <= rt * P.hub, (what, hwtv, P.hub)
            r = LAM * P.g.astype(np.float64)
            gn = np.sqrt(np.sum(gq.astype(np.float64) ** 2, axis=1))
            assert bool(np.all(gn <= r * (1.0 + 4.0 * eps))), (what, float(np.max(gn - r)))
            assert not gq[np.broadcast_to((P.g == 0)[:, None], gq.shape)].any(), what
            _untouched(keep, ("x", "xp", "xn", "gw"))
            n = keep["ws"].numel() // 3
            assert bool((keep["ws"][n + 16:] == WS_FILL).all()), what      # the call reduces through slot 0 of the workspace alone
            if pitch != (0, 0):
                _pads_are_zero(q)
        # inside the ball, on bits (once per weighting, unpitched)
        K = 1024.0
        rc, qk, _, _ = gpu_dual(nv, P, P.xbar, P.q, (K * P.g.astype(np.float64)).astype(dtype), alpha=K * ALPHA)
        assert rc == 0
        v = qk.cpu().numpy()                                               # shrink (q + sigma D x_bar), nowhere projected ...
        vn = np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=1))
        assert bool(np.all(vn[P.g > 0] < 0.5 * K * LAM * P.g[P.g > 0].astype(np.float64)))            # ... as this shows
        inside = np.broadcast_to(((vn < r * (1.0 - 8.0 * eps)) & (P.g > 0))[:, None], v.shape)
        gq = gpu_dual(nv, P, P.xbar, P.q, P.g)[1].cpu().numpy()
        assert inside.mean() >= 0.02
        np.testing.assert_array_equal(_bits(gq)[inside], _bits(v)[inside], err_msg="%s %s %s" % (scheme, shape, weighting))


def test_dual_step_is_finite_on_degenerate_inputs(nvlib):
    """finite outputs for finite inputs: an all-zero g (q = 0 afterwards) and an x_bar with zero gradient"""
    nv = nvlib
    for scheme in SCHEMES:
        for dtype in DTYPES:
            P = problem(scheme, (3, 2, 16, 20), dtype)
            rc, q, hwtv, _ = gpu_dual(nv, P, P.xbar, P.q, np.zeros_like(P.g))
            assert rc == 0 and not bool(q.any()) and hwtv == 0.0, (scheme, dtype)
            flat = np.full_like(P.xbar, 3.0)
            rc, q, hwtv, _ = gpu_dual(nv, P, flat, np.zeros_like(P.q), P.g)
            assert rc == 0 and not bool(q.any()) and hwtv == 0.0, (scheme, dtype)
            rc, q, hwtv, _ = gpu_dual(nv, P, flat, P.q, P.g)
            assert rc == 0 and bool(torch.isfinite(q).all()) and hwtv == 0.0, (scheme, dtype)


# ------------------------------------------------------------------------------------------------
# 2. hand-made slabs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_slabs_with_halo_planes_equal_the_whole_volume(nvlib, scheme, dtype):
    """planes [a, b) with the neighbours' planes of x passed by hand: q bit for bit, the scalars add up; the gap's three sums add up.  A
    missing halo plane: TV_E_HALO, nothing written."""
    nv = nvlib
    shape = (7, 3, 10, 64)
    P = problem(scheme, shape, dtype)
    rt = RTOL[dtype]
    rc, wq, whole, _ = gpu_dual(nv, P, P.xbar, P.q, P.g)
    assert rc == 0
    parts = 0.0
    for a, b in ((0, 3), (3, 4), (4, 7)):                                  # a one-plane slab in the middle
        rc, q, s, keep = gpu_dual(nv, P, P.xbar, P.q, P.g, z_range=(a, b))
        assert rc == 0 and torch.equal(q, wq[a:b]), (a, b)
        _untouched(keep, ("x", "xp", "xn", "gw"))
        parts += s
    assert abs(parts - whole) <= rt * whole
    qf = P.qn.astype(dtype)                                                # a feasible dual variable: what the dual step leaves
    ref = np_gap_hwtv(P.x, qf, P.x0, P.g.astype(np.float64), LAM, ALPHA, scheme, P.kw)
    got = gpu_gap(nv, P, P.x, qf, P.x0, P.g)
    sums = np.zeros(3)
    for a, b in ((0, 3), (3, 4), (4, 7)):
        sums += np.array(gpu_gap(nv, P, P.x, qf, P.x0, P.g, z_range=(a, b)))
    for k, scale in enumerate((ref[0], ref[1], ref[3])):
        assert abs(sums[k] - got[k]) <= rt * scale, (k, sums, got)
    sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))
    for side in sides:
        rc, q, s, keep = gpu_dual(nv, P, P.xbar, P.q, P.g, z_range=(2, 5), drop=side)
        assert rc == E_HALO and s == 123.0 and nv.lib().tv_last_error().startswith(b"x_" + side.encode()), side
        _untouched(keep, ("x", "q", "xp", "xn", "gw"))
        assert bool((keep["ws"] == WS_FILL).all())


# ------------------------------------------------------------------------------------------------
# 3. the gap against NumPy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gap_matches_numpy_and_writes_nothing(nvlib, shape, scheme, dtype):
    """(x, q) with q the feasible variable one dual step leaves (q = 0 where g = 0).  The gap is >= 0 up to the floor of its cancellation,
    16 eps * primal (tests/test_gpu_cp_huber.py)"""
    nv = nvlib
    rt, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    for weighting in WEIGHTINGS:
        P = problem(scheme, shape, dtype, weighting)
        qf = P.qn.astype(dtype)
        hub, fid, gap, terms = np_gap_hwtv(P.x, qf, P.x0, P.g.astype(np.float64), LAM, ALPHA, scheme, P.kw)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            got = gpu_gap(nv, P, P.x, qf, P.x0, P.g, pitch=pitch)
            what = "%s %s %s %s pitch %r" % (scheme, shape, np.dtype(dtype).name, weighting, pitch)
            print("%s: got %r ref %r |d gap| %.3e (tol %.3e)" % (what, got, (hub, fid, gap), abs(got[2] - gap), rt * terms))
            assert abs(got[0] - hub) <= rt * hub and abs(got[1] - fid) <= rt * fid and abs(got[2] - gap) <= rt * terms, what
            assert got[2] >= -16.0 * eps * (fid + LAM * hub), what


# ------------------------------------------------------------------------------------------------
# 4. the siblings
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_degenerate_alpha_is_tv_cp_dual_wtv_bit_for_bit(nvlib, shape, scheme, dtype):
    """sigma alpha below half an ulp of the smallest positive radius lambda * 0.25: r + sigma alpha rounds to r, the shrink factor is exactly 1
    (0 where g = 0) and q equals that of tv_cp_dual_wtv on the same input"""
    nv = nvlib
    alpha = ALPHA_DEGENERATE[dtype]
    assert SIGMA * alpha < 0.5 * np.finfo(dtype).eps * LAM * 0.25
    P = problem(scheme, shape, dtype)
    assert float(P.g[P.g > 0].min()) >= 0.25
    rc, q, _, _ = gpu_dual(nv, P, P.xbar, P.q, P.g, alpha=alpha)
    rc2, qw, _, _ = gpu_dual(nv, P, P.xbar, P.q, P.g, entry="wtv")
    assert rc == 0 and rc2 == 0 and torch.equal(q, qw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_unit_weight_agrees_with_the_huber_kernels(nvlib, shape, scheme, dtype):
    """g = 1: the dual step and the gap against tv_cp_dual_huber / tv_dual_gap_huber to the array and scalar tolerances (the two shrink factors
    round differently: no bit comparison)"""
    nv = nvlib
    rt = RTOL[dtype]
    P = problem(scheme, shape, dtype)
    one = np.ones_like(P.g)
    _, q, s, _ = gpu_dual(nv, P, P.xbar, P.q, one)
    _, qh, sh, _ = gpu_dual(nv, P, P.xbar, P.q, one, entry="huber")
    a, b = q.cpu().numpy(), qh.cpu().numpy()
    assert float(np.max(np.abs(a - b))) <= rt * float(np.max(np.abs(b))) and abs(s - sh) <= rt * sh
    got, goth = gpu_gap(nv, P, P.x, b, P.x0, one), gpu_gap(nv, P, P.x, b, P.x0, one, entry="huber")
    terms = np_gap_hwtv(P.x, b, P.x0, one.astype(np.float64), LAM, ALPHA, scheme, P.kw)[3]
    assert abs(got[0] - goth[0]) <= rt * goth[0] and abs(got[1] - goth[1]) <= rt * goth[1] and abs(got[2] - goth[2]) <= rt * terms, (got, goth)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_unit_weight_trajectory_is_huber_chambolle_pock(scheme):
    """30 fp64 iterations with g = 1 against ``HuberChambollePock`` on the kernel pair: loss rtol 1e-10, result 1e-9 max|x0|"""
    import pytv
    shape = (3, 2, 16, 20)
    kw = dict(reg_z_over_reg=0.7, reg_time=0.25)
    x0 = torch.as_tensor(noisy_square(shape).copy()).cuda()
    a = pytv.solvers.AdaptiveHuberChambollePock(x0, REG, torch.ones_like(x0), ALPHA, scheme=scheme, **kw)
    h = pytv.solvers.HuberChambollePock(x0, REG, ALPHA, scheme=scheme, **kw)
    assert a.fused is False and h.fused is False and (a.tau, a.sigma, a.theta) == (h.tau, h.sigma, h.theta) and a.g_max == 1.0
    la, lh = a.run(30), h.run(30)
    np.testing.assert_allclose(la, lh, rtol=1e-10, atol=0)
    assert float((a.result() - h.result()).abs().max()) <= 1e-9 * float(np.max(np.abs(noisy_square(shape))))
    pa, ph = a.duality_gap(), h.duality_gap()
    assert abs(pa[0] - ph[0]) <= 1e-10 * ph[0] and abs(pa[2] - ph[2]) <= 1e-10 * ph[0]
