"""The one-sweep form of the ADAPTIVE Huber-TV Chambolle-Pock iteration on the GPU (``-m gpu``): tv_cp_hwtv_sweep + tv_cp_accel_fixup through the
C-ABI against one iteration written out in NumPy float64 over the oracle's D / D^T, against the kernel pair tv_cp_dual_hwtv + tv_cp_primal_accel,
chunk / plane sub-ranges and hand-made slabs against the whole call bit for bit, a degenerate alpha against the pair, and
``AdaptiveHuberChambollePock`` on both paths against the NumPy loop and against each other.

Shapes, weightings, inputs, helpers and tolerances are those of tests/test_gpu_cp_accel_sweep.py / tests/test_gpu_cp_huber_sweep.py (the smallest
shapes that reach every seam kind, TV_ZCHUNK = 2 or 3), alpha = 2 -- with ONE change to the inputs: the deviation of x_bar from its mean 25 is
scaled by XBAR_SPREAD = 1.5.  With that module's x_bar as it is, the central scheme (differences halved) has |D x_bar|_2 > alpha at 1.9 % of the
sites of 5x9x5x68 and 1.7 % of 4x1x8x64, below the 2 % every share must reach; that share depends on x_bar and alpha alone, so no seed or
range of g moves it.  The factor was chosen on the float64 reference alone, before any GPU run: over all (scheme, shape, weighting) the
smallest share above alpha becomes 0.175 (central 4x1x8x64) and the smallest share at or below it 0.137 (hybrid 7x3x10x64, mask); 1.25
gives 0.083 / 0.261, 2.0 gives 0.394 / 0.040.  The weight g comes from a seeded generator: a third of the sites exactly
0, a third in [0.25, 1), a third in [1, 3].  Conditions on the inputs (asserted in the float64 reference, shares printed): sites on both sides
of the projection among those with r > 0, on both sides of the Huber kink, and in all three classes of g -- each share at least 2 %
(tests/test_cp_hwtv_inputs.py checks every case on the CPU, without a GPU).
Tolerances: arrays to RTOL = 1e-5 (fp32) / 1e-11 (fp64) of the array's max, scalars to the same RTOL of the reference, summed partial scalars
to 1e-12; solver results fp64 1e-9 * max|x0|, fp32 rtol 1e-5 / atol 2e-3; fp64 loss histories rtol 1e-10."""
import functools
import types

import numpy as np
import pytest
import torch

import test_gpu_cp_accel_sweep as acc
from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_accel_sweep import (CASE_IDS, CASES, E_HALO, FID_BOTH, FID_OF_INPUT, FLAG_MODES, LAM, OUTPUTS, RTOL, SIGMA, SLAB_CASES, SLAB_IDS,
                                     TAU, THETA, WEIGHTINGS, _close12, _explicit_pitch, _first_difference, _geom, _pads_are_zero, _scalars,
                                     _storage, chunk_partitions, fixup, plane_partitions, z_channels)
from test_gpu_cp_huber import REG, huber, noisy_square, np_linear_steps

pytestmark = pytest.mark.gpu

ALPHA = 2.0
ALPHA_DEGENERATE = {np.float32: 1e-9, np.float64: 1e-18}
MIN_SHARE = 0.02
XBAR_SPREAD = 1.5


@pytest.fixture(scope="module")
def nvlib():
    import pytv  # noqa: F401
    from pytv import _native as nv
    return nv


def weights(shape, seed=5):
    """g of the issue: a third of the sites exactly 0, a third in [0.25, 1), a third in [1, 3] (float64; exactly representable classes)"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, size=shape)
    u = rng.random(shape)
    return np.where(cls == 0, 0.0, np.where(cls == 1, 0.25 + 0.75 * u, 1.0 + 2.0 * u))


def np_dual_hwtv(q, dx, g, sigma, lam, alpha):
    """the dual update in float64: (q_new, v, |v|_2, r); g broadcasts over the channel axis"""
    r = lam * g[:, None]
    shrink = np.where(r > 0, r / (r + sigma * alpha), 0.0)
    v = shrink * (q + sigma * dx)
    n = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(r > 0, np.where(n > r, r / np.where(n > 0, n, 1.0), 1.0), 0.0)
    return v * s, v, n, r


def np_gap_hwtv(x, q, x0, g, lam, alpha, scheme, kw):
    """(sum g h_alpha(|D x|), 1/2 |x - x0|^2, gap, sum |terms|) in float64, the gap site by site"""
    x, q, x0 = (np.asarray(a, dtype=np.float64) for a in (x, q, x0))
    dx = orc.D(x, scheme, **kw)
    rr = x - x0 + orc.D_T(q, scheme, **kw)
    h = huber(np.sqrt(np.sum(dx * dx, axis=1)), alpha)
    r = lam * g
    dot, qq = np.sum(q * dx, axis=1), np.sum(q * q, axis=1)
    conj = np.where(r > 0, alpha * qq / (2.0 * np.where(r > 0, r, 1.0)), 0.0)
    gap = np.sum(0.5 * rr * rr) + np.sum(r * h + conj - dot)
    terms = np.sum(0.5 * rr * rr) + np.sum(r * h + conj + np.abs(dot))
    return float(np.sum(g * h)), float(0.5 * np.sum((x - x0) ** 2)), float(gap), float(terms)


# ------------------------------------------------------------------------------------------------
# inputs (those of test_gpu_cp_accel_sweep.Problem, plus g) and the float64 reference of one iteration: computed once, never modified
# ------------------------------------------------------------------------------------------------
class HwtvProblem:
    def __init__(self, scheme, shape, dtype, weighting):
        A = acc.problem(scheme, shape, dtype, weighting)
        self.scheme, self.shape, self.dtype, self.kw = A.scheme, A.shape, A.dtype, A.kw
        f8 = np.float64
        self.x0, self.x, self.q, self.nd = A.x0, A.x, A.q, A.nd
        self.xbar = (25.0 + XBAR_SPREAD * (A.xbar.astype(f8) - 25.0)).astype(dtype)          # (module docstring)
        self.g = weights(self.shape).astype(dtype)
        g = self.g.astype(f8)
        dxb = orc.D(self.xbar.astype(f8), scheme, **self.kw)
        self.qn, v, nrm, r = np_dual_hwtv(self.q.astype(f8), dxb, g, SIGMA, LAM, ALPHA)
        n = np.sqrt(np.sum(dxb * dxb, axis=1))
        nrm, r = nrm[:, 0], r[:, 0]
        self.shares = dict(outside=float((nrm > r)[r > 0].sum() / r.size), inside=float(((nrm > 0) & (nrm <= r)).sum() / r.size),
                           below=float((n <= ALPHA).mean()), above=float((n > ALPHA).mean()),
                           g0=float((g == 0).mean()), g1=float(((g >= 0.25) & (g < 1)).mean()), g2=float((g >= 1).mean()))
        print("shares", scheme, shape, weighting, self.shares)
        assert min(self.shares.values()) >= MIN_SHARE, (scheme, shape, weighting, self.shares)
        x, x0 = self.x.astype(f8), self.x0.astype(f8)
        self.xn = (x - TAU * orc.D_T(self.qn, scheme, **self.kw) + TAU * x0) / (1.0 + TAU)
        self.xb = self.xn + THETA * (self.xn - x)
        self.hub = float(np.sum(g * huber(n, ALPHA)))
        self.fid_in = 0.5 * float(np.sum((x - x0) ** 2))
        self.fid_out = 0.5 * float(np.sum((self.xn - x0) ** 2))


_PROBLEMS = {}


def problem(scheme, shape, dtype, weighting="plain"):
    key = (scheme, tuple(shape), np.dtype(dtype).name, weighting)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = HwtvProblem(scheme, shape, dtype, weighting)
    return _PROBLEMS[key]


def state(g, P, sep, a=0, b=None):
    b = P.shape[0] if b is None else b
    s = acc.state(g, P, sep, a, b)
    s["gw"] = g.new_image(b - a)
    s["gw"].copy_(torch.as_tensor(np.ascontiguousarray(P.g[a:b])))
    return s


def sweep(nv, g, s, xp, xn, flags, cb, cc, sc, alpha=ALPHA):
    ptr = nv.ptr
    return nv.lib().tv_cp_hwtv_sweep(g.ref, ptr(s["xbar"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["qo"]), ptr(s["x0"]), ptr(s["x"]), ptr(s["xbo"]),
                                     ptr(s["gw"]), SIGMA, LAM, alpha, TAU, THETA, flags, cb, cc, sc[0:1].data_ptr(), sc[1:3].data_ptr(),
                                     ptr(g.workspace()), nv.current_stream(g.device))


def run_ranges(nv, g, s, flags, chunk_ranges, plane_ranges, xh=(None, None), qh=(None, None), alpha=ALPHA):
    sw, fx = _scalars(len(chunk_ranges), 3), _scalars(len(plane_ranges), 1)
    for i, (cb, cc) in enumerate(chunk_ranges):
        nv.check(sweep(nv, g, s, xh[0], xh[1], flags, cb, cc, sw[i], alpha))
    for i, (zb, zn) in enumerate(plane_ranges):
        nv.check(fixup(nv, g, s, qh[0], qh[1], flags, zb, zn, fx[i]))
    return sw.sum(dim=0).cpu().numpy(), float(fx.sum())


def run_pair(nv, g, s, alpha=ALPHA):
    """tv_cp_dual_hwtv (on x_bar, q in place) + tv_cp_primal_accel on a state of ``state(..., sep=False)``; returns (hwtv, fid)"""
    ptr = nv.ptr
    sc = _scalars(1, 2)[0]
    st, ws = nv.current_stream(g.device), ptr(g.workspace())
    nv.check(nv.lib().tv_cp_dual_hwtv(g.ref, ptr(s["xbar"]), None, None, ptr(s["q"]), ptr(s["gw"]), SIGMA, LAM, alpha, sc[0:1].data_ptr(), ws, st))
    nv.check(nv.lib().tv_cp_primal_accel(g.ref, ptr(s["q"]), None, None, ptr(s["x"]), ptr(s["xbar"]), ptr(s["x0"]), TAU, THETA,
                                         sc[1:2].data_ptr(), ws, st))
    return float(sc[0]), float(sc[1])


def check_scalars(P, flags, sw, fx, what):
    rt = RTOL[P.dtype]
    assert abs(sw[0] - P.hub) <= rt * P.hub, ("hwtv", what, sw[0], P.hub)
    if flags == 0:
        assert abs(sw[1] + fx - P.fid_out) <= rt * P.fid_out, ("fid", what, sw[1], fx, P.fid_out)
        return
    assert abs(sw[1] - P.fid_in) <= rt * P.fid_in, ("fid of the input", what, sw[1], P.fid_in)
    if flags & FID_BOTH:
        assert abs(sw[2] + fx - P.fid_out) <= rt * P.fid_out, ("fid of the output", what, sw[2], fx, P.fid_out)
    else:
        assert fx == 0.0, ("fix-up without x0", what, fx)


# ------------------------------------------------------------------------------------------------
# 1. one iteration against the oracle, three flag modes; inputs never written, pads stay zero
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_one_iteration_matches_the_oracle(nvlib, scheme, case, tvopt):
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 3 if shape[0] >= 6 else 2)
    rt = RTOL[dtype]
    for weighting in WEIGHTINGS:
        P = problem(scheme, shape, dtype, weighting)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            g = _geom(nv, P, pitch)
            assert nv.lib().tv_cp_fused_supported(g.ref) == 1
            for flags in FLAG_MODES:
                sep = flags != 0
                what = "%s %s %s pitch %r flags %d" % (scheme, shape, weighting, pitch, flags)
                s = state(g, P, sep)
                before = {k: _storage(s[k]).clone() for k in ("x0", "xbar", "gw") + (("q",) if sep else ())}
                sw, fx = run_ranges(nv, g, s, flags, [(0, -1)], [(0, -1)])
                for name, want in (("x", P.xn), ("xbo", P.xb), ("qo", P.qn)):
                    got = s[name].cpu().numpy()
                    tol = rt * float(np.max(np.abs(want)))
                    err = float(np.max(np.abs(got - want)))
                    print("%s: %s max|d| %.3e (tol %.3e)" % (what, name, err, tol))
                    assert got.dtype == dtype and err <= tol, (what, name, err, tol)
                print("%s: hwtv %.12e (ref %.12e) fid %r + %.12e" % (what, sw[0], P.hub, sw[1:].tolist(), fx))
                check_scalars(P, flags, sw, fx, what)
                # exactness: g = 0 sites end with q == 0 in every channel
                qo = s["qo"].cpu().numpy()
                assert not qo[np.broadcast_to((P.g == 0)[:, None], qo.shape)].any(), what
                for k, v in before.items():
                    assert torch.equal(_storage(s[k]), v), (what, k, "input written to")
                if pitch != (0, 0):
                    for name in OUTPUTS:
                        _pads_are_zero(s[name])


# ------------------------------------------------------------------------------------------------
# 2. against the kernel pair, also with a degenerate alpha
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sweep_and_fixup_agree_with_the_kernel_pair(nvlib, scheme, case, tvopt):
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 2)
    rt = RTOL[dtype]
    deg = ALPHA_DEGENERATE[dtype]
    assert SIGMA * deg < 0.5 * np.finfo(dtype).eps * LAM * 0.25
    for weighting, alpha in [(w, ALPHA) for w in WEIGHTINGS] + [("plain", deg)]:
        P = problem(scheme, shape, dtype, weighting)
        g = _geom(nv, P)
        s = state(g, P, False)
        sw, fx = run_ranges(nv, g, s, 0, [(0, -1)], [(0, -1)], alpha=alpha)
        r = state(g, P, False)
        hub, fid = run_pair(nv, g, r, alpha)
        for mine, theirs in (("qo", "q"), ("x", "x"), ("xbo", "xbar")):
            a, b = s[mine].cpu().numpy(), r[theirs].cpu().numpy()
            err, tol = float(np.max(np.abs(a - b))), rt * float(np.max(np.abs(b)))
            print("%s %s %s alpha %g: %s max|d| %.3e (tol %.3e)" % (scheme, shape, weighting, alpha, mine, err, tol))
            assert err <= tol, (weighting, alpha, mine, err, tol)
        print("%s %s %s: hwtv %.15e pair %.15e fid %.15e pair %.15e" % (scheme, shape, weighting, sw[0], hub, sw[1] + fx, fid))
        assert abs(sw[0] - hub) <= rt * hub and abs(sw[1] + fx - fid) <= rt * fid, (weighting, sw, fx, hub, fid)


# ------------------------------------------------------------------------------------------------
# 3. chunk / plane ranges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_chunk_and_plane_ranges_equal_the_whole_call(nvlib, scheme, case, zchunk, tvopt):
    nv = nvlib
    tvopt("TV_ZCHUNK", zchunk)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    g = _geom(nv, P)
    nz, zc = shape[0], nv.lib().tv_cp_zchunk(g.ref)
    assert zc == min(int(zchunk), nz)
    nch = (nz + zc - 1) // zc
    cparts, pparts = chunk_partitions(nch), plane_partitions(nz, zc)
    assert len(cparts) == 3 and len(pparts) == 3
    for flags in FLAG_MODES:
        sep = flags != 0
        s0 = state(g, P, sep)
        sw0, fx0 = run_ranges(nv, g, s0, flags, [(0, -1)], [(0, -1)])
        check_scalars(P, flags, sw0, fx0, "whole call, TV_ZCHUNK=%s" % zchunk)
        for cpart, ppart in zip(cparts, pparts):
            s1 = state(g, P, sep)
            sw1, fx1 = run_ranges(nv, g, s1, flags, cpart, ppart)
            for k in OUTPUTS:
                assert torch.equal(s1[k], s0[k]), (flags, k, cpart, ppart, _first_difference(s1[k], s0[k]))
            assert _close12(sw1[0], sw0[0]) and _close12(sw1[1], sw0[1]) and (not (flags & FID_BOTH) or _close12(sw1[2], sw0[2])), (flags, cpart, sw1, sw0)
            assert _close12(fx1, fx0) if flags != FID_OF_INPUT else fx1 == 0.0, (flags, ppart, fx1, fx0)


# ------------------------------------------------------------------------------------------------
# 4. slabs by hand
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", SLAB_CASES, ids=SLAB_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_slabs_cut_on_the_chunk_seams_equal_unsharded(nvlib, scheme, case, zchunk, tvopt):
    """every slab swept with the neighbouring slabs' planes of x_bar as halos (g has none), then fixed up with the boundary plane of the
    neighbour's q_out: x, x_bar_out and q_out are those of the unsharded call bit for bit.  An interior slab without a halo plane its scheme
    reads: TV_E_HALO, nothing written."""
    nv = nvlib
    tvopt("TV_ZCHUNK", zchunk)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    nz = shape[0]
    g = _geom(nv, P)
    zc = nv.lib().tv_cp_zchunk(g.ref)
    cuts = tuple(range(0, nz, zc)) + (nz,)
    assert len(cuts) >= 3 and all(c % zc == 0 for c in cuts[1:-1])
    slabs = list(zip(cuts[:-1], cuts[1:]))
    ch_back, ch_fwd = z_channels(scheme)
    XB = torch.as_tensor(P.xbar).cuda()
    for flags in (0, FID_OF_INPUT | FID_BOTH):
        sep = flags != 0
        s0 = state(g, P, sep)
        sw0, fx0 = run_ranges(nv, g, s0, flags, [(0, -1)], [(0, -1)])
        geoms = [_geom(nv, P, a=a, b=b) for a, b in slabs]
        states = [state(geoms[i], P, sep, a, b) for i, (a, b) in enumerate(slabs)]
        sw, fx = _scalars(len(slabs), 3), _scalars(len(slabs), 1)
        for i, (a, b) in enumerate(slabs):
            xp = XB[a - 1].clone() if a > 0 else None
            xn = XB[b].clone() if b < nz else None
            nv.check(sweep(nv, geoms[i], states[i], xp, xn, flags, 0, -1, sw[i]))
        for i, (a, b) in enumerate(slabs):
            hp = states[i - 1]["qo"][-1, ch_back].clone() if a > 0 else None
            hn = states[i + 1]["qo"][0, ch_fwd].clone() if b < nz else None
            nv.check(fixup(nv, geoms[i], states[i], hp, hn, flags, 0, -1, fx[i]))
        for k in OUTPUTS:
            got = torch.cat([s[k] for s in states])
            assert torch.equal(got, s0[k]), (flags, k, cuts, _first_difference(got, s0[k]))
        tot = sw.sum(dim=0).cpu().numpy()
        assert _close12(tot[0], sw0[0]) and _close12(tot[1], sw0[1]) and _close12(float(fx.sum()), fx0), (flags, tot, sw0, float(fx.sum()), fx0)
        assert not (flags & FID_BOTH) or _close12(tot[2], sw0[2]), (flags, tot, sw0)
    a, b = 1, nz - 1
    gi = _geom(nv, P, a=a, b=b)
    plane = XB[0].clone()
    x_sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))
    for side in x_sides:
        s = state(gi, P, True, a, b)
        before = {k: v.clone() for k, v in s.items()}
        sc = _scalars(1, 3, 123.0)
        assert sweep(nv, gi, s, None if side == "prev" else plane, None if side == "next" else plane, 0, 0, -1, sc[0]) == E_HALO, side
        torch.cuda.synchronize()
        assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), side


# ------------------------------------------------------------------------------------------------
# 4b. hybrid volumes of 7 frames (fp32) and 6 frames (fp64): no single-window instantiation, one ragged window of the windowed kernel
# ------------------------------------------------------------------------------------------------
ROUTED_CASES = [((5, 7, 9, 68), np.float32), ((5, 6, 9, 66), np.float64)]


@pytest.mark.parametrize("case", ROUTED_CASES, ids=["5x7x9x68-float32", "5x6x9x66-float64"])
def test_hybrid_volumes_without_a_single_window_instantiation(nvlib, case, tvopt):
    """cphwt_windowed (tv_fused.h): against NumPy in the three flag modes, against the pair, and chunk / plane ranges bit for bit"""
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 2)
    rt = RTOL[dtype]
    nz = shape[0]
    for weighting in WEIGHTINGS:
        P = problem("hybrid", shape, dtype, weighting)
        g = _geom(nv, P)
        assert nv.lib().tv_cp_fused_supported(g.ref) == 1
        for flags in FLAG_MODES:
            s = state(g, P, flags != 0)
            sw, fx = run_ranges(nv, g, s, flags, [(0, -1)], [(0, -1)])
            for name, want in (("x", P.xn), ("xbo", P.xb), ("qo", P.qn)):
                err, tol = float(np.max(np.abs(s[name].cpu().numpy() - want))), rt * float(np.max(np.abs(want)))
                print("%s %s flags %d: %s max|d| %.3e (tol %.3e)" % (shape, weighting, flags, name, err, tol))
                assert err <= tol, (weighting, flags, name, err, tol)
            check_scalars(P, flags, sw, fx, "%s %s flags %d" % (shape, weighting, flags))
    P = problem("hybrid", shape, dtype)
    g = _geom(nv, P)
    s0, r = state(g, P, False), state(g, P, False)
    sw0, fx0 = run_ranges(nv, g, s0, 0, [(0, -1)], [(0, -1)])
    hub, fid = run_pair(nv, g, r)
    for mine, theirs in (("qo", "q"), ("x", "x"), ("xbo", "xbar")):
        a, b = s0[mine].cpu().numpy(), r[theirs].cpu().numpy()
        assert float(np.max(np.abs(a - b))) <= rt * float(np.max(np.abs(b))), mine
    assert abs(sw0[0] - hub) <= rt * hub and abs(sw0[1] + fx0 - fid) <= rt * fid
    nch = (nz + 1) // 2
    for cpart, ppart in zip(chunk_partitions(nch), plane_partitions(nz, 2)):
        s1 = state(g, P, False)
        sw1, fx1 = run_ranges(nv, g, s1, 0, cpart, ppart)
        for k in OUTPUTS:
            assert torch.equal(s1[k], s0[k]), (k, cpart, ppart, _first_difference(s1[k], s0[k]))
        assert _close12(sw1[0], sw0[0]) and _close12(sw1[1], sw0[1]) and _close12(fx1, fx0)


# ------------------------------------------------------------------------------------------------
# 5. the solver
# ------------------------------------------------------------------------------------------------
SOLVER_SHAPES = [(7, 3, 10, 64), (5, 9, 5, 68)]
SOLVER_SCHEMES = ["hybrid", "upwind"]
SOLVER_DTYPES = [np.float64, np.float32]
N_ITER = 20
KW = dict(reg_z_over_reg=0.7, reg_time=0.25)


def np_hwtv_cp(x0, g, n_iter, lam, alpha, scheme, kw):
    """n_iter iterations of Algorithm 3 from the start with delta = alpha / (lam g_max); returns (x, loss, q)"""
    x0 = np.asarray(x0, dtype=np.float64)
    gmax = float(g.max()) if float(g.max()) > 0 else 1.0
    tau, sigma, theta = np_linear_steps(orc.normal_spectral_bound(scheme, x0.shape, **kw), 1.0, alpha / (lam * gmax))
    x, xb, q = x0.copy(), x0.copy(), np.zeros_like(orc.D(x0, scheme, **kw))
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        dxb = orc.D(xb, scheme, **kw)
        q = np_dual_hwtv(q, dxb, g, sigma, lam, alpha)[0]
        xn = (x - tau * orc.D_T(q, scheme, **kw) + tau * x0) / (1.0 + tau)
        xb = xn + theta * (xn - x)
        x = xn
        loss[k] = 0.5 * np.sum((x - x0) ** 2) + lam * np.sum(g * huber(np.sqrt(np.sum(dxb * dxb, axis=1)), alpha))
    return x, loss, q


@functools.lru_cache(maxsize=None)
def np_state(shape, scheme, f32_input, n_iter):
    x0, g = noisy_square(shape), weights(shape)
    if f32_input:
        x0, g = x0.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
    x, loss, q = np_hwtv_cp(x0, g, n_iter, REG, ALPHA, scheme, KW)
    hub, fid, gap, _ = np_gap_hwtv(x, q, x0, g, REG, ALPHA, scheme, KW)
    return x, loss, (fid + REG * hub, gap)


def _solver(pytv, shape, dtype, scheme, fused, g=None):
    g = weights(shape) if g is None else g
    cp = pytv.solvers.AdaptiveHuberChambollePock(torch.as_tensor(noisy_square(shape).astype(dtype)).cuda(), REG, torch.as_tensor(g.astype(dtype)).cuda(),
                                                 ALPHA, scheme=scheme, **KW)
    cp.set_fused(fused)
    assert cp.fused is fused
    return cp


def _assert_x_close(x, want, dtype, shape, what):
    print("%s: max|dx| %.3e" % (what, float(np.max(np.abs(x - want)))))
    if dtype == np.float64:
        assert float(np.max(np.abs(x - want))) <= 1e-9 * float(np.max(np.abs(noisy_square(shape)))), what
    else:
        np.testing.assert_allclose(x, want, rtol=1e-5, atol=2e-3, err_msg=what)


@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SOLVER_SCHEMES)
@pytest.mark.parametrize("shape", SOLVER_SHAPES)
def test_solver_paths_agree_with_numpy_and_each_other(shape, scheme, dtype, tvopt):
    """20 iterations on the sweep, on the pair, switching path every 5 iterations, and again after reset(): x against the float64 NumPy loop,
    the fp64 loss history to rtol 1e-10, duality_gap() against the NumPy certificate and path against path"""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    f64 = dtype == np.float64
    wx, wloss, (wprimal, wgap) = np_state(shape, scheme, not f64, N_ITER)
    runs = {}
    for name in ("sweep", "pair", "switching"):
        cp = _solver(pytv, shape, dtype, scheme, name != "pair")
        loss = None
        if name == "switching":
            for block in range(N_ITER // 5):
                cp.set_fused(block % 2 == 0)
                cp.run(5, record_loss=False)
        else:
            loss = cp.run(N_ITER)
            assert loss.shape == (N_ITER,) and np.isfinite(loss).all()
            if f64:
                np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
        assert cp.it == N_ITER
        what = "%s %s %s %s" % (shape, scheme, np.dtype(dtype).name, name)
        runs[name] = (cp.result().cpu().numpy().copy(), cp.duality_gap(), loss)
        _assert_x_close(runs[name][0], wx, dtype, shape, what)
        if name != "switching":                                          # reset(): the same run again, the path kept
            cp.reset()
            assert cp.it == 0 and cp.fused is (name == "sweep") and torch.equal(cp.x, cp.x0) and not bool(cp.q.any())
            cp.run(N_ITER, record_loss=False)
            _assert_x_close(cp.result().cpu().numpy(), runs[name][0], dtype, shape, what + " after reset")
    rt = 1e-9 if f64 else 1e-5
    np.testing.assert_allclose(runs["sweep"][2], runs["pair"][2], rtol=rt, atol=0)
    p0, d0, g0 = runs["sweep"][1]
    print("%s %s %s sweep %r numpy primal %.12e gap %.6e" % (shape, scheme, np.dtype(dtype).name, runs["sweep"][1], wprimal, wgap))
    if f64:                                                              # the NumPy certificate after the same 20 iterations
        assert abs(p0 - wprimal) <= rt * wprimal and abs(g0 - wgap) <= rt * wprimal
    for name in ("pair", "switching"):
        p1, d1, g1 = runs[name][1]
        assert abs(p0 - p1) <= rt * abs(p1) and abs(d0 - d1) <= rt * abs(d1) and abs(g0 - g1) <= rt * abs(p1), (name, runs["sweep"][1], runs[name][1])


@pytest.mark.parametrize("scheme", SOLVER_SCHEMES)
@pytest.mark.parametrize("shape", SOLVER_SHAPES)
def test_run_until_converges_on_both_paths_fp64(shape, scheme, tvopt):
    """run_until(1e-6) converges on both paths and reports the gap of the NumPy certificate evaluated at the solver's own (x, q)"""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    x0, g = noisy_square(shape), weights(shape)
    for fused in (True, False):
        cp = _solver(pytv, shape, np.float64, scheme, fused)
        _, info = cp.run_until(1e-6, 2000, 20)
        assert cp.fused is fused and info["converged"] is True and info["gap"] <= 1e-6 * info["primal"], info
        hub, fid, gap, _ = np_gap_hwtv(cp.x.cpu().numpy(), cp.q.cpu().numpy(), x0, g, REG, ALPHA, scheme, KW)
        print(shape, scheme, fused, info, "numpy primal %.15e gap %.15e" % (fid + REG * hub, gap))
        assert abs(info["primal"] - (fid + REG * hub)) <= 1e-9 * (fid + REG * hub)
        assert abs(info["gap"] - gap) <= 1e-9 * (fid + REG * hub)          # the gap cancels from terms of the primal's size


def test_set_fused_refuses_nx_40_and_a_sharded_slab():
    import pytv
    shape = (3, 2, 16, 40)
    cp = pytv.solvers.AdaptiveHuberChambollePock(torch.as_tensor(noisy_square(shape).copy()).cuda(), REG, torch.as_tensor(weights(shape)).cuda(), ALPHA)
    assert cp.fused is False
    with pytest.raises(ValueError, match="one-sweep"):
        cp.set_fused(True)
    assert cp.fused is False
    cp.run(3)
    assert cp.it == 3
    cp = _solver(pytv, (7, 3, 10, 64), np.float64, "hybrid", True)
    own = cp.slab
    cp.slab = types.SimpleNamespace(sharded=True)
    try:
        with pytest.raises(ValueError, match="unsharded"):
            cp.set_fused(True)
        assert cp.fused is True
        cp.set_fused(None)
        assert cp.fused is False
    finally:
        cp.slab = own


def test_construction_default_follows_TV_FUSED_MIN_KVOXELS_in_the_sweep_schemes():
    """``ChambollePock``'s rule in the schemes of ``SWEEP_DEFAULT_SCHEMES`` (those whose sweep measured faster than the pair by more than the
    pair's spread, profiles/adaptive_huber_bench.txt); the pair in the others whatever the option says.  (Other GPU test modules lower
    TV_FUSED_MIN_KVOXELS to 0 for the whole process: the option is unset here by hand and put back.)"""
    import pytv
    from pytv import _native as nv
    cls = pytv.solvers.AdaptiveHuberChambollePock
    assert set(cls.SWEEP_DEFAULT_SCHEMES) <= set(SCHEMES)
    shape = (7, 3, 10, 64)
    x0, g = torch.as_tensor(noisy_square(shape).copy()).cuda(), torch.as_tensor(weights(shape)).cuda()
    saved = nv.get_option("TV_FUSED_MIN_KVOXELS", -1)
    try:
        for scheme in SCHEMES:
            sweeps = scheme in cls.SWEEP_DEFAULT_SCHEMES
            nv.set_option("TV_FUSED_MIN_KVOXELS", None)
            cp = cls(x0, REG, g, ALPHA, scheme=scheme)                    # 13440 voxels against the default 16 Mi
            assert cp.fused is False
            nv.set_option("TV_FUSED_MIN_KVOXELS", 1)
            assert cls(x0, REG, g, ALPHA, scheme=scheme).fused is sweeps, scheme
            cp.set_fused(None)
            assert cp.fused is sweeps, scheme                             # None re-evaluates the default rule
            cp.set_fused(True)
            assert cp.fused is True                                       # the choice stays the caller's in every scheme
    finally:
        nv.set_option("TV_FUSED_MIN_KVOXELS", None if saved < 0 else saved)


@pytest.mark.parametrize("fused", [True, False], ids=["sweep", "pair"])
@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
def test_protected_region_and_all_zero_weights(dtype, fused, tvopt):
    """a g = 0 block whose neighbouring sites have g = 0 too stays within 8 eps max|x0| of x0 after 50 iterations; an all-zero g returns x0"""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    shape = (7, 3, 10, 64)
    g = np.ones(shape)
    g[1:6, :, 2:8, 16:48] = 0.0                                  # the block and a one-site rim of zero weight around its core
    cp = _solver(pytv, shape, dtype, "hybrid", fused, g)
    cp.run(50, record_loss=False)
    x, x0 = cp.result().cpu().numpy(), noisy_square(shape).astype(dtype)
    core = (slice(2, 5), slice(None), slice(3, 7), slice(17, 47))
    bound = 8.0 * np.finfo(dtype).eps * float(np.max(np.abs(x0)))
    print("protected core: max|x - x0| %.3e (bound %.3e)" % (float(np.max(np.abs(x[core] - x0[core]))), bound))
    assert float(np.max(np.abs(x[core] - x0[core]))) <= bound
    assert float(np.max(np.abs(x - x0))) > 1.0                           # the background was smoothed
    cp = _solver(pytv, shape, dtype, "hybrid", fused, np.zeros(shape))
    assert cp.g_max == 0.0 and np.isfinite([cp.tau, cp.sigma, cp.theta]).all()
    cp.run(5, record_loss=False)
    assert float(np.max(np.abs(cp.result().cpu().numpy() - x0))) <= bound and not bool(cp.q.any())


def test_constructor_refusals():
    import pytv
    shape = (3, 2, 16, 20)
    x0, g = torch.as_tensor(noisy_square(shape).copy()).cuda(), weights(shape)
    cls = pytv.solvers.AdaptiveHuberChambollePock
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            cls(x0, REG, g, alpha)
    for reg in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="regularization"):
            cls(x0, reg, g, ALPHA)
    bad = g.copy()
    bad[0, 0, 0, 0] = -1e-3
    with pytest.raises(ValueError, match="reg_weights"):
        cls(x0, REG, bad, ALPHA)
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="reg_weights"):
        cls(x0, REG, bad, ALPHA)
    with pytest.raises(ValueError, match="reg_weights"):
        cls(x0, REG, g[:, :, :, :-1], ALPHA)


@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
def test_denoise_tv_adaptive_huber_is_the_same_on_either_default(dtype, tvopt, monkeypatch):
    import pytv
    tvopt("TV_ZCHUNK", 2)
    img = noisy_square((1, 1, 24, 64))[0, 0].astype(dtype)
    g = weights((24, 64)).astype(dtype)
    out = {}
    monkeypatch.setattr(pytv.solvers.AdaptiveHuberChambollePock, "SWEEP_DEFAULT_SCHEMES", ("upwind",))       # whatever was measured: both defaults
    for fused, kvox in ((True, 1), (False, 1 << 30)):
        tvopt("TV_FUSED_MIN_KVOXELS", kvox)
        probe = pytv.solvers.AdaptiveHuberChambollePock(torch.as_tensor(img.reshape(1, 1, 24, 64)).cuda(), REG,
                                                        torch.as_tensor(g.reshape(1, 1, 24, 64)).cuda(), ALPHA, scheme="upwind")
        assert probe.fused is fused
        out[fused] = pytv.denoise_tv_adaptive_huber(img, weight=REG, reg_weights=g, alpha=ALPHA, rel_gap=1e-14, max_num_iter=N_ITER, scheme="upwind")
    assert out[True].dtype == dtype and out[True].shape == img.shape
    if dtype == np.float64:
        assert float(np.max(np.abs(out[True] - out[False]))) <= 1e-9 * float(np.max(np.abs(img)))
    else:
        np.testing.assert_allclose(out[True], out[False], rtol=1e-5, atol=2e-3)
    assert float(np.max(np.abs(out[True] - img))) > 1.0
