"""The one-sweep form of the accelerated Chambolle-Pock iteration on the GPU (``-m gpu``): tv_cp_accel_sweep + tv_cp_accel_fixup through the
C-ABI against one iteration written out in NumPy float64 over the oracle's D / D^T, the dual part against tv_cp_sweep bit for bit, chunk /
plane sub-ranges and hand-made slabs against the whole call bit for bit, and ``AcceleratedChambollePock.set_fused(True)`` against the NumPy
loop and against the kernel pair.

Shapes: the smallest that reach every seam kind (tests/test_gpu_sweep_ranges.py), TV_ZCHUNK = 2 or 3 so that z-chunk seams exist.
Tolerances: arrays to RTOL = 1e-5 (fp32) / 1e-11 (fp64) of the array's max and scalars to the same RTOL of the reference -- what
tests/test_gpu_cp_accel.py uses for tv_cp_primal_accel; summed partial scalars to 1e-12 (test_gpu_sweep_ranges.py)."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
SIGMA, LAM, TAU, THETA = 0.5, 5.0, 0.3, 0.37
SENT = 7.0                                                 # what output arrays hold before a call
E_HALO = -2
FID_OF_INPUT, FID_BOTH = 1, 2
FLAG_MODES = (0, FID_OF_INPUT, FID_OF_INPUT | FID_BOTH)

CASES = [((7, 3, 10, 64), np.float32),       # one block tile; ny ragged against the 8-row wave tile
         ((7, 3, 10, 64), np.float64),
         ((6, 2, 9, 320), np.float32),       # crosses the 256-column block tile, a partial tile follows
         ((5, 9, 5, 68), np.float32),        # M > 8: one time-window seam; partial wave tile
         ((5, 9, 5, 66), np.float64),        # the same in fp64 (2 columns per lane)
         ((4, 1, 8, 64), np.float32)]        # M = 1, no time axis
CASE_IDS = ["%s-%s" % ("x".join(map(str, s)), np.dtype(d).name) for s, d in CASES]
SLAB_CASES = [c for c in CASES if c[0][0] in (7, 5)]
SLAB_IDS = ["%s-%s" % ("x".join(map(str, s)), np.dtype(d).name) for s, d in SLAB_CASES]
WEIGHTINGS = ("plain", "mask", "time_factor", "weight_vol")


def _case_kw(name, shape):
    """the four weightings of tests/test_gpu_cp_accel.py"""
    rng = np.random.default_rng(17)
    if name == "mask":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=rng.random((1, 1) + shape[2:]) < 0.4, factor_reg_static=3.0)
    if name == "time_factor":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random((1, 1) + shape[2:])))
    if name == "weight_vol":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random(shape)))
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


def _explicit_pitch(shape, dtype):
    lane = 16 // np.dtype(dtype).itemsize
    rp = -(-(shape[3] + 4) // lane) * lane                              # nx + 4 rounded up to 16 bytes
    return rp, shape[2] * rp + 8


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _storage(t):
    """the whole allocation behind a (possibly pitched) view, pads included"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def _pads_are_zero(t):
    pads = _storage(t).clone()
    pads.as_strided(t.shape, t.stride()).zero_()
    assert not bool(pads.any())                                        # what is not a voxel is a pad


def z_channels(scheme):
    """(ch_back, ch_fwd): the z channel whose adjoint looks backwards / forwards -- the planes tv_DT names y_prev / y_next"""
    per = 2 if scheme == "hybrid" else 1
    return 2 * per, 2 * per + (1 if scheme == "hybrid" else 0)


@pytest.fixture(scope="module")
def nvlib():
    import pytv  # noqa: F401
    from pytv import _native as nv
    return nv


# ------------------------------------------------------------------------------------------------
# inputs and the float64 reference of one iteration: computed once per (scheme, shape, dtype, weighting), never modified
# ------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, scheme, shape, dtype, weighting):
        self.scheme, self.shape, self.dtype = scheme, tuple(shape), dtype
        self.kw = kw = _case_kw(weighting, self.shape)
        rng = np.random.default_rng(17)
        f8 = np.float64
        self.x0 = (50.0 * rng.random(shape)).astype(dtype)
        self.xbar = (25.0 + rng.standard_normal(shape)).astype(dtype)
        self.x = (self.xbar + 0.5 * rng.standard_normal(shape)).astype(dtype)
        dxb = orc.D(self.xbar.astype(f8), scheme, **kw)
        self.nd = dxb.shape[1]
        self.q = (LAM / np.sqrt(self.nd) * rng.standard_normal(dxb.shape)).astype(dtype)      # |q| scatters around lambda
        v = self.q.astype(f8) + SIGMA * dxb
        nrm = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        assert (nrm > LAM).any() and (nrm < LAM).any()                 # both branches of the projection (a condition on the input)
        x, x0 = self.x.astype(f8), self.x0.astype(f8)
        self.qn = v / np.maximum(1.0, nrm / LAM)
        self.xn = (x - TAU * orc.D_T(self.qn, scheme, **kw) + TAU * x0) / (1.0 + TAU)
        self.xb = self.xn + THETA * (self.xn - x)
        self.tv = float(orc.compute_L21_norm(dxb))
        self.fid_in = 0.5 * float(np.sum((x - x0) ** 2))
        self.fid_out = 0.5 * float(np.sum((self.xn - x0) ** 2))


_PROBLEMS = {}


def problem(scheme, shape, dtype, weighting="plain"):
    key = (scheme, tuple(shape), np.dtype(dtype).name, weighting)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(scheme, shape, dtype, weighting)
    return _PROBLEMS[key]


def _geom(nv, P, pitch=(0, 0), a=0, b=None):
    """geometry of the planes [a, b) of the volume (plain weighting when it is a proper slab)"""
    nzg = P.shape[0]
    b = nzg if b is None else b
    return nv.Geometry((b - a,) + P.shape[1:], P.scheme, _tdt(P.dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1], **P.kw)


def state(g, P, sep, a=0, b=None):
    """fresh device arrays for the planes [a, b) with the geometry's pitches: inputs copied, outputs filled with SENT (pads stay zero)"""
    b = P.shape[0] if b is None else b

    def img(arr):
        t = g.new_image(b - a)
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    s = dict(xbar=img(P.xbar[a:b]), x=img(P.x[a:b]), x0=img(P.x0[a:b]), q=g.new_grad(b - a), xbo=g.new_image(b - a))
    s["q"].copy_(torch.as_tensor(np.ascontiguousarray(P.q[a:b])))
    s["xbo"].fill_(SENT)
    if sep:
        s["qo"] = g.new_grad(b - a)
        s["qo"].fill_(SENT)
    else:
        s["qo"] = s["q"]
    return s


OUTPUTS = ("x", "xbo", "qo")


def sweep(nv, g, s, xp, xn, flags, cb, cc, sc):
    """sc: three fp64 words (tv, fid[0], fid[1] under TV_CP_FID_BOTH); returns the status"""
    ptr = nv.ptr
    return nv.lib().tv_cp_accel_sweep(g.ref, ptr(s["xbar"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["qo"]), ptr(s["x0"]), ptr(s["x"]), ptr(s["xbo"]),
                                      SIGMA, LAM, TAU, THETA, flags, cb, cc, sc[0:1].data_ptr(), sc[1:3].data_ptr(), ptr(g.workspace()),
                                      nv.current_stream(g.device))


def fixup(nv, g, s, hp, hn, flags, zb, zn, sc):
    """sc: one fp64 word.  The lagged fidelity alone (TV_CP_FID_OF_INPUT): the fix-up is given no x0"""
    ptr = nv.ptr
    x0 = None if flags == FID_OF_INPUT else s["x0"]
    return nv.lib().tv_cp_accel_fixup(g.ref, ptr(s["qo"]), ptr(hp), ptr(hn), ptr(s["x"]), ptr(s["xbo"]), ptr(x0), TAU, THETA, zb, zn,
                                      sc.data_ptr(), ptr(g.workspace()), nv.current_stream(g.device))


def _scalars(n, width, fill=0.0):
    return torch.full((max(n, 1), width), fill, dtype=torch.float64, device="cuda")


def run_ranges(nv, g, s, flags, chunk_ranges, plane_ranges, xh=(None, None), qh=(None, None)):
    """the sweep over each chunk range, then the fix-up over each plane range, every call with scalar slots of its own;
    returns the summed sweep scalars [3] and the summed fix-up scalar"""
    sw, fx = _scalars(len(chunk_ranges), 3), _scalars(len(plane_ranges), 1)
    for i, (cb, cc) in enumerate(chunk_ranges):
        nv.check(sweep(nv, g, s, xh[0], xh[1], flags, cb, cc, sw[i]))
    for i, (zb, zn) in enumerate(plane_ranges):
        nv.check(fixup(nv, g, s, qh[0], qh[1], flags, zb, zn, fx[i]))
    return sw.sum(dim=0).cpu().numpy(), float(fx.sum())


def check_scalars(P, flags, sw, fx, what):
    """*tv and *fid in the three flag modes (sweep + fix-up summed where that applies) against the reference sums"""
    rt = RTOL[P.dtype]
    assert abs(sw[0] - P.tv) <= rt * P.tv, ("tv", what, sw[0], P.tv)
    if flags == 0:
        assert abs(sw[1] + fx - P.fid_out) <= rt * P.fid_out, ("fid", what, sw[1], fx, P.fid_out)
        return
    assert abs(sw[1] - P.fid_in) <= rt * P.fid_in, ("fid of the input", what, sw[1], P.fid_in)
    if flags & FID_BOTH:
        assert abs(sw[2] + fx - P.fid_out) <= rt * P.fid_out, ("fid of the output", what, sw[2], fx, P.fid_out)
    else:
        assert fx == 0.0, ("fix-up without x0", what, fx)


def _first_difference(a, b):
    d = torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b))))
    if d.numel() == 0:
        return None
    i = tuple(int(v) for v in d[0])
    return i, float(a[i]), float(b[i]), int(d.shape[0])


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
                print("%s: tv %.12e fid %r + %.12e" % (what, sw[0], sw[1:].tolist(), fx))
                check_scalars(P, flags, sw, fx, what)
                for k, v in before.items():
                    assert torch.equal(_storage(s[k]), v), (what, k, "input written to")      # the whole allocation: pad columns included
                if pitch != (0, 0):
                    for name in OUTPUTS:
                        _pads_are_zero(s[name])


# ------------------------------------------------------------------------------------------------
# 2. the dual part is that of tv_cp_sweep
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dual_update_is_bit_identical_to_tv_cp_sweep(nvlib, scheme, case, tvopt):
    """q_out bit for bit and *tv equal.  (The sum of squares under the TV partial has a pinned order of roundings in k_cp_fused,
    sumsq_slots_pinned: written as s + o * o the compiler contracted its first two terms differently in the two instantiations of
    6x2x9x320-float32-hybrid, 73303.87914095819 against 73303.87914644182.)"""
    nv = nvlib
    shape, dtype = case
    tvopt("TV_ZCHUNK", 2)
    P = problem(scheme, shape, dtype)
    g = _geom(nv, P)
    ptr = nv.ptr
    s = state(g, P, True)
    sw, _ = run_ranges(nv, g, s, 0, [(0, -1)], [(0, -1)])
    r = state(g, P, True)                                              # tv_cp_sweep: x_in = x_bar, the same q, sigma and lambda; its p is r["x"]
    sc = _scalars(1, 3)[0]
    nv.check(nv.lib().tv_cp_sweep(g.ref, ptr(r["xbar"]), None, None, ptr(r["q"]), ptr(r["qo"]), ptr(r["x0"]), ptr(r["x"]), ptr(r["xbo"]), SIGMA, LAM,
                                  0.05, 1.0, 0, 0, -1, sc[0:1].data_ptr(), sc[1:3].data_ptr(), ptr(g.workspace()), nv.current_stream(g.device)))
    assert torch.equal(s["qo"], r["qo"]), _first_difference(s["qo"], r["qo"])
    assert sw[0] == float(sc[0]), (sw[0], float(sc[0]))


# ------------------------------------------------------------------------------------------------
# 3. chunk / plane ranges
# ------------------------------------------------------------------------------------------------
def chunk_partitions(nch):
    parts = [[(k, 1) for k in reversed(range(nch))]]                         # every chunk on its own, in reverse order
    if nch >= 2:
        na = (nch - 2 + 1) // 2
        nb = nch - 2 - na
        parts.append([(1, na), (0, 1), (nch - 1, 1), (1 + na, nb)])          # the interior-first order of ChambollePock's slabs
        h = nch // 2
        parts.append([(0, h), (h, nch - h)])                                 # a two-way split at a chunk in the middle
    return parts


def plane_partitions(nz, zc):
    parts = [[(k, 1) for k in reversed(range(nz))]]                          # every plane on its own
    if nz >= 2:
        parts.append([(1, nz - 2), (0, 1), (nz - 1, 1)])
        mid = [s for s in range(1, nz) if s % zc != 0]                        # a split in the middle of a chunk
        if mid:
            s0 = min(mid, key=lambda s: abs(s - nz / 2.0))
            parts.append([(s0, nz - s0), (0, s0)])
    return parts


def _close12(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


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
    q_sides = {"upwind": ("prev",), "downwind": ("next",)}.get(scheme, ("prev", "next"))        # ... and their adjoint q(z-1)
    for side in x_sides:
        s = state(gi, P, True, a, b)
        before = {k: v.clone() for k, v in s.items()}
        sc = _scalars(1, 3, 123.0)
        assert sweep(nv, gi, s, None if side == "prev" else plane, None if side == "next" else plane, 0, 0, -1, sc[0]) == E_HALO, side
        torch.cuda.synchronize()
        assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), side
    for side in q_sides:
        s = state(gi, P, True, a, b)
        nv.check(sweep(nv, gi, s, plane, plane, 0, 0, -1, _scalars(1, 3)[0]))
        before = {k: v.clone() for k, v in s.items()}
        sc = _scalars(1, 1, 123.0)
        assert fixup(nv, gi, s, None if side == "prev" else plane, None if side == "next" else plane, 0, 0, -1, sc[0]) == E_HALO, side
        torch.cuda.synchronize()
        assert all(torch.equal(s[k], before[k]) for k in s) and sc.item() == 123.0, side


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (a copy of tests/test_gpu_cp_accel.py's)
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
def np_trajectory(shape, scheme, n_iter, f32_input=False):
    x0 = square_plus_noise(shape)
    if f32_input:
        x0 = x0.astype(np.float32).astype(np.float64)
    return np_accel(x0, n_iter, 25.0, scheme, _kw_of(shape))


def _solver(pytv, shape, dtype, scheme, fused=None):
    cp = pytv.solvers.AcceleratedChambollePock(torch.as_tensor(square_plus_noise(shape).astype(dtype)).cuda(), 25.0, scheme=scheme, **_kw_of(shape))
    if fused is not None:
        cp.set_fused(fused)
        assert cp.fused is fused
    return cp


# ------------------------------------------------------------------------------------------------
# 5. solver trajectory
# ------------------------------------------------------------------------------------------------
TRAJ_SHAPES = [(1, 1, 24, 64), (4, 2, 16, 64), (3, 9, 8, 64)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme, tvopt):
    import pytv
    tvopt("TV_ZCHUNK", 2)
    wx, wloss = np_trajectory(shape, scheme, 40)
    cp = _solver(pytv, shape, np.float64, scheme, True)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    pair = _solver(pytv, shape, np.float64, scheme, False)
    ploss = pair.run(40)
    print("%s %s: loss rel %.3e  against the pair %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)),
                                                                        np.max(np.abs(loss / ploss - 1.0)), np.max(np.abs(x - wx))))
    assert cp.it == 40 and cp.fused is True and pair.fused is False
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(square_plus_noise(shape))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    np.testing.assert_allclose(loss, ploss, rtol=1e-12, atol=0)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme, tvopt):
    """the bounds of tests/test_gpu_cp_accel.py::test_solver_trajectory_fp32: loss rtol 1e-5; result rtol 1e-5, atol 2e-3 (pixel values of O(100))"""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    wx, wloss = np_trajectory(shape, scheme, 40, f32_input=True)
    cp = _solver(pytv, shape, np.float32, scheme, True)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


# ------------------------------------------------------------------------------------------------
# 6. switching paths between iterations, reset
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_switching_paths_between_iterations_and_reset(scheme, dtype, tvopt):
    """20 iterations on the pair, set_fused(True), 20 more: the history and the iterate equal those of 40 iterations on EITHER path (and the
    NumPy loop) to the bounds of the trajectory tests -- fp64: loss 1e-12 path to path, 1e-10 to NumPy, x 1e-9 max|x0|; fp32: loss rtol 1e-5,
    x rtol 1e-5 / atol 2e-3."""
    import pytv
    tvopt("TV_ZCHUNK", 2)
    shape = (4, 2, 16, 64)
    f64 = dtype == np.float64
    wx, wloss = np_trajectory(shape, scheme, 40, f32_input=not f64)
    cp = _solver(pytv, shape, dtype, scheme, False)
    loss = [cp.run(20)]
    cp.set_fused(True)
    assert cp.fused is True and cp.it == 20
    loss = np.concatenate(loss + [cp.run(20)])
    x = cp.result().cpu().numpy()
    assert cp.it == 40
    xmax = float(np.max(np.abs(square_plus_noise(shape))))
    refs = [("numpy", wx, wloss, 1e-10)]
    for fused in (False, True):                                           # 40 iterations on either path
        whole = _solver(pytv, shape, dtype, scheme, fused)
        wl = whole.run(40)
        assert whole.fused is fused and whole.it == 40
        refs.append(("fused=%s" % fused, whole.result().cpu().numpy(), wl, 1e-12))
    for name, rx, rloss, rt in refs:
        print("%s %s against %s: loss rel %.3e  max|dx| %.3e" % (scheme, np.dtype(dtype).name, name, np.max(np.abs(loss / rloss - 1.0)),
                                                               np.max(np.abs(x - rx))))
        if f64:
            assert float(np.max(np.abs(x - rx))) <= 1e-9 * xmax, name
            np.testing.assert_allclose(loss, rloss, rtol=rt, atol=0, err_msg=name)
        else:
            np.testing.assert_allclose(x, rx, rtol=1e-5, atol=2e-3, err_msg=name)
            np.testing.assert_allclose(loss, rloss, rtol=1e-5, atol=0, err_msg=name)
    cp.reset()
    assert cp.it == 0 and cp.fused is True
    assert torch.equal(cp.x, cp.x0) and torch.equal(cp.x_bar, cp.x0) and not bool(cp.q.any())
    again = cp.run(40)                                                    # ... and the whole run on the sweep path from there
    np.testing.assert_array_equal(again, refs[2][2])
    cp.set_fused(False)
    assert cp.fused is False


# ------------------------------------------------------------------------------------------------
# 7. certificate
# ------------------------------------------------------------------------------------------------
def test_run_until_certifies_on_the_sweep_path(tvopt):
    import pytv
    tvopt("TV_ZCHUNK", 2)
    shape, scheme = (1, 1, 48, 64), "hybrid"
    sw, pair = _solver(pytv, shape, np.float64, scheme, True), _solver(pytv, shape, np.float64, scheme, False)
    _, i_s = sw.run_until(1e-3, 400)
    _, i_p = pair.run_until(1e-3, 400)
    print("sweep", i_s, "pair", i_p)
    assert i_s["converged"] is True and i_p["converged"] is True and i_s["gap"] <= 1e-3 * i_s["primal"]
    assert abs(i_s["iterations"] - i_p["iterations"]) <= 10               # one check_every
    n = max(sw.it, pair.it)                                               # the certificates of the same iterate
    sw.run(n - sw.it)
    pair.run(n - pair.it)
    for a, b in zip(sw.duality_gap(), pair.duality_gap()):
        assert abs(a - b) <= 1e-6 * abs(b), (sw.duality_gap(), pair.duality_gap())


# ------------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------------
def test_set_fused_refuses_a_geometry_the_sweep_does_not_take():
    import pytv
    shape = (3, 2, 16, 20)                                                # nx < 64
    cp = _solver(pytv, shape, np.float64, "hybrid")
    assert cp.fused is False
    with pytest.raises(ValueError, match="one-sweep"):
        cp.set_fused(True)
    assert cp.fused is False
    wx, wloss = np_trajectory(shape, "hybrid", 5)
    np.testing.assert_allclose(cp.run(5), wloss, rtol=1e-10, atol=0)      # still usable, on the pair
    cp.set_fused(None)
    assert cp.fused is False


def test_set_fused_refuses_a_sharded_slab():
    """the sweep / exchange / fix-up schedule of slabs is not built: on a sharded slab set_fused(True) raises and None chooses the pair,
    whatever the geometry (here one the sweep supports, with the slab object standing in for one rank of several)"""
    import types
    import pytv
    cp = _solver(pytv, (4, 2, 16, 64), np.float64, "hybrid", True)
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
