"""The one-sweep form of the Huber-TV Chambolle-Pock iteration on the GPU (``-m gpu``): tv_cp_huber_sweep + tv_cp_accel_fixup through the C-ABI
against one iteration written out in NumPy float64 over the oracle's D / D^T, against the kernel pair tv_cp_dual_huber + tv_cp_primal_accel,
with a degenerate alpha against tv_cp_accel_sweep bit for bit, chunk / plane sub-ranges and hand-made slabs against the whole call bit for
bit, and ``HuberChambollePock.set_fused(True)`` against the NumPy loop and against the kernel pair.

Shapes, weightings, inputs and helpers are those of tests/test_gpu_cp_accel_sweep.py (the smallest shapes that reach every seam kind,
TV_ZCHUNK = 2 or 3 so that z-chunk seams exist), alpha = 2.
Tolerances: arrays to RTOL = 1e-5 (fp32) / 1e-11 (fp64) of the array's max and scalars to the same RTOL of the reference; summed partial
scalars to 1e-12; solver results as tests/test_gpu_cp_accel_sweep.py compares its own solver: fp64 1e-9 * max|x0|, fp32 rtol 1e-5 / atol 2e-3."""
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
                                     _storage, chunk_partitions, fixup, plane_partitions, state, z_channels)
from test_gpu_cp_huber import REG, huber, noisy_square, np_huber_cp, np_huber_gap

pytestmark = pytest.mark.gpu

ALPHA = 2.0
# sigma alpha / lambda below half an ulp of 1 in the dtype: shrink = 1 / (1 + sigma alpha / lambda), formed in double, rounds to exactly 1
ALPHA_DEGENERATE = {np.float32: 1e-9, np.float64: 1e-18}
HUB_AGAINST_TV = {np.float32: 1e-6, np.float64: 1e-12}


@pytest.fixture(scope="module")
def nvlib():
    import pytv  # noqa: F401
    from pytv import _native as nv
    return nv


# ------------------------------------------------------------------------------------------------
# inputs (those of test_gpu_cp_accel_sweep.Problem) and the float64 reference of one Huber-TV iteration: computed once, never modified
# ------------------------------------------------------------------------------------------------
class HuberProblem:
    def __init__(self, scheme, shape, dtype, weighting):
        A = acc.problem(scheme, shape, dtype, weighting)
        self.scheme, self.shape, self.dtype, self.kw = A.scheme, A.shape, A.dtype, A.kw
        self.x0, self.xbar, self.x, self.q, self.nd = A.x0, A.xbar, A.x, A.q, A.nd
        f8 = np.float64
        dxb = orc.D(self.xbar.astype(f8), scheme, **self.kw)
        v = (self.q.astype(f8) + SIGMA * dxb) / (1.0 + SIGMA * ALPHA / LAM)
        nrm = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        n = np.sqrt(np.sum(dxb * dxb, axis=1))
        # two conditions on the INPUT: both sides of the projection and both sides of the Huber kink occur
        assert (nrm > LAM).any() and (nrm < LAM).any(), (scheme, shape, weighting, float(nrm.min()), float(nrm.max()))
        assert (n <= ALPHA).any() and (n > ALPHA).any(), (scheme, shape, weighting, float(n.min()), float(n.max()))
        self.shares = (float((nrm > LAM).mean()), float((n > ALPHA).mean()))
        x, x0 = self.x.astype(f8), self.x0.astype(f8)
        self.qn = v / np.maximum(1.0, nrm / LAM)
        self.xn = (x - TAU * orc.D_T(self.qn, scheme, **self.kw) + TAU * x0) / (1.0 + TAU)
        self.xb = self.xn + THETA * (self.xn - x)
        self.hub = float(np.sum(huber(n, ALPHA)))
        self.fid_in = 0.5 * float(np.sum((x - x0) ** 2))
        self.fid_out = 0.5 * float(np.sum((self.xn - x0) ** 2))


_PROBLEMS = {}


def problem(scheme, shape, dtype, weighting="plain"):
    key = (scheme, tuple(shape), np.dtype(dtype).name, weighting)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = HuberProblem(scheme, shape, dtype, weighting)
    return _PROBLEMS[key]


def sweep(nv, g, s, xp, xn, flags, cb, cc, sc, alpha=ALPHA):
    """sc: three fp64 words (hub, fid[0], fid[1] under TV_CP_FID_BOTH); returns the status"""
    ptr = nv.ptr
    return nv.lib().tv_cp_huber_sweep(g.ref, ptr(s["xbar"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["qo"]), ptr(s["x0"]), ptr(s["x"]), ptr(s["xbo"]),
                                      SIGMA, LAM, alpha, TAU, THETA, flags, cb, cc, sc[0:1].data_ptr(), sc[1:3].data_ptr(), ptr(g.workspace()),
                                      nv.current_stream(g.device))


def run_ranges(nv, g, s, flags, chunk_ranges, plane_ranges, xh=(None, None), qh=(None, None), alpha=ALPHA):
    """the Huber sweep over each chunk range, then tv_cp_accel_fixup (same tau, theta) over each plane range, every call with scalar slots of
    its own; returns the summed sweep scalars [3] and the summed fix-up scalar"""
    sw, fx = _scalars(len(chunk_ranges), 3), _scalars(len(plane_ranges), 1)
    for i, (cb, cc) in enumerate(chunk_ranges):
        nv.check(sweep(nv, g, s, xh[0], xh[1], flags, cb, cc, sw[i], alpha))
    for i, (zb, zn) in enumerate(plane_ranges):
        nv.check(fixup(nv, g, s, qh[0], qh[1], flags, zb, zn, fx[i]))
    return sw.sum(dim=0).cpu().numpy(), float(fx.sum())


def check_scalars(P, flags, sw, fx, what):
    """*hub and *fid in the three flag modes (sweep + fix-up summed where that applies) against the reference sums"""
    rt = RTOL[P.dtype]
    assert abs(sw[0] - P.hub) <= rt * P.hub, ("hub", what, sw[0], P.hub)
    if flags == 0:
        assert abs(sw[1] + fx - P.fid_out) <= rt * P.fid_out, ("fid", what, sw[1], fx, P.fid_out)
        return
    assert abs(sw[1] - P.fid_in) <= rt * P.fid_in, ("fid of the input", what, sw[1], P.fid_in)
    if flags & FID_BOTH:
        assert abs(sw[2] + fx - P.fid_out) <= rt * P.fid_out, ("fid of the output", what, sw[2], fx, P.fid_out)
    else:
        assert fx == 0.0, ("fix-up without x0", what, fx)


# ------------------------------------------------------------------------------------------------
# 1. one iteration against the oracle
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
                sep = flags != 0                                          # q ping-pong in the lagged modes, in place otherwise
                what = "%s %s %s pitch %r flags %d" % (scheme, shape, weighting, pitch, flags)
                s = state(g, P, sep)
                before = {k: _storage(s[k]).clone() for k in ("x0", "xbar") + (("q",) if sep else ())}
                sw, fx = run_ranges(nv, g, s, flags, [(0, -1)], [(0, -1)])
                for name, want in (("x", P.xn), ("xbo", P.xb), ("qo", P.qn)):
                    got = s[name].cpu().numpy()
                    tol = rt * float(np.max(np.abs(want)))
                    err = float(np.max(np.abs(got - want)))
                    print("%s: %s max|d| %.3e (tol %.3e)" % (what, name, err, tol))
                    assert got.dtype == dtype and err <= tol, (what, name, err, tol)
                print("%s: hub %.12e (ref %.12e) fid %r + %.12e" % (what, sw[0], P.hub, sw[1:].tolist(), fx))
                check_scalars(P, flags, sw, fx, what)
                for k, v in before.items():
                    assert torch.equal(_storage(s[k]), v), (what, k, "input written to")      # the whole allocation: pad columns included
                if pitch != (0, 0):
                    for name in OUTPUTS:
                        _pads_are_zero(s[name])


# ------------------------------------------------------------------------------------------------
# 2. against the kernel pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sweep_and_fixup_agree_with_the_kernel_pair(nvlib, scheme, case, tvopt):
    """the same state through tv_cp_dual_huber (on x_bar, q in place) + tv_cp_primal_accel: q, x, x_bar and the Huber sum agree"""
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 2)
    rt = RTOL[dtype]
    ptr = nv.ptr
    for weighting in WEIGHTINGS:
        P = problem(scheme, shape, dtype, weighting)
        g = _geom(nv, P)
        s = state(g, P, False)
        sw, fx = run_ranges(nv, g, s, 0, [(0, -1)], [(0, -1)])
        r = state(g, P, False)
        sc = _scalars(1, 2)[0]
        st, ws = nv.current_stream(g.device), ptr(g.workspace())
        nv.check(nv.lib().tv_cp_dual_huber(g.ref, ptr(r["xbar"]), None, None, ptr(r["q"]), SIGMA, LAM, ALPHA, sc[0:1].data_ptr(), ws, st))
        nv.check(nv.lib().tv_cp_primal_accel(g.ref, ptr(r["q"]), None, None, ptr(r["x"]), ptr(r["xbar"]), ptr(r["x0"]), TAU, THETA,
                                             sc[1:2].data_ptr(), ws, st))
        for mine, theirs in (("qo", "q"), ("x", "x"), ("xbo", "xbar")):
            a, b = s[mine].cpu().numpy(), r[theirs].cpu().numpy()
            err, tol = float(np.max(np.abs(a - b))), rt * float(np.max(np.abs(b)))
            print("%s %s %s: %s max|d| %.3e (tol %.3e)" % (scheme, shape, weighting, mine, err, tol))
            assert err <= tol, (weighting, mine, err, tol)
        hub, fid = float(sc[0]), float(sc[1])
        print("%s %s %s: hub %.15e pair %.15e fid %.15e pair %.15e" % (scheme, shape, weighting, sw[0], hub, sw[1] + fx, fid))
        assert abs(sw[0] - hub) <= rt * hub and abs(sw[1] + fx - fid) <= rt * fid, (weighting, sw, fx, hub, fid)


# ------------------------------------------------------------------------------------------------
# 3. degenerate alpha: the shipped accelerated sweep, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_degenerate_alpha_is_the_accelerated_sweep_bit_for_bit(nvlib, scheme, case, tvopt):
    """shrink rounds to exactly 1 and no site lies below the kink: q_out, x and x_bar_out are those of tv_cp_accel_sweep + tv_cp_accel_fixup bit for
    bit, and *hub = *tv - (alpha / 2) * sites, i.e. *tv to far less than the bound.  Nothing but the dual multiply and the partial differs."""
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 2)
    alpha = ALPHA_DEGENERATE[dtype]
    assert SIGMA * alpha / LAM < 0.5 * np.finfo(dtype).eps
    assert dtype(1.0 / (1.0 + SIGMA * alpha / LAM)) == dtype(1.0)
    P = problem(scheme, shape, dtype)
    g = _geom(nv, P)
    for flags in (0, FID_OF_INPUT | FID_BOTH):
        sep = flags != 0
        s = state(g, P, sep)
        sw, fx = run_ranges(nv, g, s, flags, [(0, -1)], [(0, -1)], alpha=alpha)
        r = state(g, P, sep)
        rsw, rfx = acc.run_ranges(nv, g, r, flags, [(0, -1)], [(0, -1)])
        for k in OUTPUTS:
            assert torch.equal(s[k], r[k]), (flags, k, _first_difference(s[k], r[k]))
        print("%s %s flags %d: hub %.15e tv %.15e" % (scheme, shape, flags, sw[0], rsw[0]))
        assert abs(sw[0] - rsw[0]) <= HUB_AGAINST_TV[dtype] * rsw[0], (sw[0], rsw[0])
        assert np.array_equal(sw[1:], rsw[1:]) and fx == rfx, (sw, rsw, fx, rfx)


# ------------------------------------------------------------------------------------------------
# 4. chunk / plane ranges
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
# 5. slabs by hand
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", SLAB_CASES, ids=SLAB_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_slabs_cut_on_the_chunk_seams_equal_unsharded(nvlib, scheme, case, zchunk, tvopt):
    """every slab swept with the neighbouring slabs' planes of x_bar as halos, then fixed up with the boundary plane of the neighbour's q_out
    in the channel tv_DT names for that side: x, x_bar_out and q_out are those of the unsharded call bit for bit.  An interior slab without a
    halo plane its scheme reads: TV_E_HALO, nothing written."""
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
    # a missing halo plane on an interior slab (any cut will do for a refusal)
    a, b = 1, nz - 1
    gi = _geom(nv, P, a=a, b=b)
    plane = XB[0].clone()
    x_sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))        # forward differences read x(z+1)
    for side in x_sides:
        s = state(gi, P, True, a, b)
        before = {k: v.clone() for k, v in s.items()}
        sc = _scalars(1, 3, 123.0)
        assert sweep(nv, gi, s, None if side == "prev" else plane, None if side == "next" else plane, 0, 0, -1, sc[0]) == E_HALO, side
        torch.cuda.synchronize()
        assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), side


# ------------------------------------------------------------------------------------------------
# 6. the solver
# ------------------------------------------------------------------------------------------------
SOLVER_SHAPES = [(7, 3, 10, 64), (5, 9, 5, 68)]
SOLVER_SCHEMES = ["hybrid", "upwind"]
SOLVER_DTYPES = [np.float64, np.float32]
N_ITER = 20


def _kw_of(shape):
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


def _x0(shape, dtype):
    return noisy_square(shape).astype(dtype)


@functools.lru_cache(maxsize=None)
def np_state(shape, scheme, f32_input, n_iter):
    """(x, (primal, gap)) of the NumPy loop after n_iter iterations"""
    x0 = noisy_square(shape)
    if f32_input:
        x0 = x0.astype(np.float32).astype(np.float64)
    x, _, (_, _, q) = np_huber_cp(x0, n_iter, REG, ALPHA, scheme, _kw_of(shape))
    return x, np_huber_gap(x, q, x0, REG, ALPHA, scheme, _kw_of(shape))


def _solver(pytv, shape, dtype, scheme, fused):
    cp = pytv.solvers.HuberChambollePock(torch.as_tensor(_x0(shape, dtype)).cuda(), REG, ALPHA, scheme=scheme, **_kw_of(shape))
    cp.set_fused(fused)
    assert cp.fused is fused
    return cp


def _assert_x_close(x, want, dtype, shape, what):
    """the bounds test_gpu_cp_accel_sweep.py uses for its own solver comparison"""
    print("%s: max|dx| %.3e" % (what, float(np.max(np.abs(x - want)))))
    if dtype == np.float64:
        assert float(np.max(np.abs(x - want))) <= 1e-9 * float(np.max(np.abs(noisy_square(shape)))), what
    else:
        np.testing.assert_allclose(x, want, rtol=1e-5, atol=2e-3, err_msg=what)


@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SOLVER_SCHEMES)
@pytest.mark.parametrize("shape", SOLVER_SHAPES)
def test_solver_paths_agree_with_numpy_and_each_other(shape, scheme, dtype, tvopt):
    """20 iterations on the sweep, on the pair, and switching path every 5 iterations: x against the float64 NumPy loop, duality_gap() path
    against path.  The certificate's bound: primal and dual to the relative tolerance of the dtype (1e-9 / 1e-5); the gap, a sum whose terms
    are of the size of the primal and cancel (``HuberChambollePock._GAP_DOC``: absolute error of order eps * P), to that tolerance of the
    PRIMAL."""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    f64 = dtype == np.float64
    wx, (wprimal, wgap) = np_state(shape, scheme, not f64, N_ITER)
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
        assert cp.it == N_ITER
        runs[name] = (cp.result().cpu().numpy(), cp.duality_gap(), loss)
        _assert_x_close(runs[name][0], wx, dtype, shape, "%s %s %s %s" % (shape, scheme, np.dtype(dtype).name, name))
    rt = 1e-9 if f64 else 1e-5
    np.testing.assert_allclose(runs["sweep"][2], runs["pair"][2], rtol=rt, atol=0)           # the loss history (slots F and F + 1 summed)
    for name in ("pair", "switching"):
        (p0, d0, g0), (p1, d1, g1) = runs["sweep"][1], runs[name][1]
        print("%s %s %s sweep %r %s %r numpy primal %.12e gap %.6e" % (shape, scheme, np.dtype(dtype).name, (p0, d0, g0), name, (p1, d1, g1), wprimal, wgap))
        assert abs(p0 - p1) <= rt * abs(p1) and abs(d0 - d1) <= rt * abs(d1) and abs(g0 - g1) <= rt * abs(p1), (name, runs["sweep"][1], runs[name][1])


@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("scheme", SOLVER_SCHEMES)
@pytest.mark.parametrize("shape", SOLVER_SHAPES)
def test_run_until_converges_on_both_paths(shape, scheme, dtype, tvopt):
    import pytv
    tvopt("TV_ZCHUNK", 2)
    info = {}
    for fused in (True, False):
        cp = _solver(pytv, shape, dtype, scheme, fused)
        _, info[fused] = cp.run_until(1e-4, 200)
        assert cp.fused is fused
    print(shape, scheme, np.dtype(dtype).name, "sweep", info[True], "pair", info[False])
    for i in info.values():
        assert i["converged"] is True and i["gap"] <= 1e-4 * i["primal"] and i["iterations"] < 200
    assert abs(info[True]["iterations"] - info[False]["iterations"]) <= 10            # one check_every


def test_set_fused_contract(tvopt):
    """set_fused between iterations leaves the state alone; reset() keeps the choice; x_bar_alt appears on first use"""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    cp = _solver(pytv, (7, 3, 10, 64), np.float64, "hybrid", False)
    assert cp.x_bar_alt is None
    cp.run(3)
    snap = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
    cp.set_fused(True)
    assert cp.fused is True and cp.it == 3 and all(torch.equal(a, b) for a, b in zip(snap, (cp.x, cp.x_bar, cp.q)))
    cp.run(2)
    assert cp.x_bar_alt is not None and cp.x_bar_alt.shape == cp.x_bar.shape and cp.it == 5
    cp.reset()
    assert cp.fused is True and cp.it == 0 and torch.equal(cp.x, cp.x0) and torch.equal(cp.x_bar, cp.x0) and not bool(cp.q.any())
    cp.set_fused(False)
    assert cp.fused is False


def test_set_fused_refuses_nx_40_and_a_sharded_slab():
    import pytv
    x0 = torch.as_tensor(noisy_square((3, 2, 16, 40)).copy()).cuda()
    cp = pytv.solvers.HuberChambollePock(x0, REG, ALPHA, scheme="hybrid")
    assert cp.fused is False
    with pytest.raises(ValueError, match="one-sweep"):
        cp.set_fused(True)
    assert cp.fused is False
    cp.run(3)                                                             # still usable, on the pair
    assert cp.it == 3
    # a sharded slab (the slab object standing in for one rank of several), on a geometry the sweep supports
    cp = _solver(pytv, (7, 3, 10, 64), np.float64, "hybrid", True)
    own = cp.slab
    cp.slab = types.SimpleNamespace(sharded=True)
    try:
        with pytest.raises(ValueError, match="unsharded"):
            cp.set_fused(True)
        assert cp.fused is True                                           # a refused call changes nothing
        cp.set_fused(None)
        assert cp.fused is False
    finally:
        cp.slab = own
    cp.set_fused(True)
    assert cp.fused is True


def test_construction_default_follows_TV_FUSED_MIN_KVOXELS():
    """(other GPU test modules lower TV_FUSED_MIN_KVOXELS to 0 for the whole process: the option is unset here by hand and put back)"""
    import pytv
    from pytv import _native as nv
    shape = (7, 3, 10, 64)
    x0 = torch.as_tensor(noisy_square(shape).copy()).cuda()
    saved = nv.get_option("TV_FUSED_MIN_KVOXELS", -1)
    nv.set_option("TV_FUSED_MIN_KVOXELS", None)
    try:
        cp = pytv.solvers.HuberChambollePock(x0, REG, ALPHA, scheme="upwind")        # 13440 voxels against the default 16 Mi
        assert cp.fused is False
        nv.set_option("TV_FUSED_MIN_KVOXELS", 1)
        on = pytv.solvers.HuberChambollePock(x0, REG, ALPHA, scheme="upwind")
        assert on.fused is True
        cp.set_fused(None)
        assert cp.fused is True                                           # None re-evaluates the default rule
    finally:
        nv.set_option("TV_FUSED_MIN_KVOXELS", None if saved < 0 else saved)


@pytest.mark.parametrize("dtype", SOLVER_DTYPES, ids=["float64", "float32"])
def test_denoise_tv_huber_is_the_same_on_either_default(dtype, tvopt):
    """``denoise_tv_huber`` runs the solver's construction default: with TV_FUSED_MIN_KVOXELS = 1 that is the sweep for this image, with a
    threshold no image reaches the pair.  The same 20 iterations on either path (a relative gap no 20 iterations reach, so both stop on the
    iteration limit)."""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    img = noisy_square((1, 1, 24, 64))[0, 0].astype(dtype)
    out = {}
    for fused, kvox in ((True, 1), (False, 1 << 30)):
        tvopt("TV_FUSED_MIN_KVOXELS", kvox)
        probe = pytv.solvers.HuberChambollePock(torch.as_tensor(img.reshape(1, 1, 24, 64)).cuda(), REG, ALPHA, scheme="upwind")
        assert probe.fused is fused
        out[fused] = pytv.denoise_tv_huber(img, weight=REG, alpha=ALPHA, rel_gap=1e-14, max_num_iter=N_ITER)
    assert out[True].dtype == dtype and out[True].shape == img.shape
    if dtype == np.float64:
        assert float(np.max(np.abs(out[True] - out[False]))) <= 1e-9 * float(np.max(np.abs(img)))
    else:
        np.testing.assert_allclose(out[True], out[False], rtol=1e-5, atol=2e-3)
    assert float(np.max(np.abs(out[True] - img))) > 1.0                    # it did denoise
