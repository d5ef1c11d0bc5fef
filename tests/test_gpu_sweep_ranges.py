"""Chunk / plane sub-ranges and slab halos of the one-sweep entry points at the C-ABI (include/pytv4d.h): tv_cp_fused / tv_cp_sweep +
tv_cp_fixup, tv_admm_fused / tv_admm_sweep + tv_admm_fixup, tv_cpop_fused + tv_cpop_fixup -- one process, one iteration, every
output array compared plane by plane.

  1. a sweep cut into chunk ranges and a fix-up cut into plane ranges give the arrays of the whole call bit for bit, and partial
     scalars that sum to the whole call's;
  2. only the first / last chunk reads x_prev / x_next, only plane 0 / nz-1 reads q_prev / q_next (t_prev / t_next): NaN planes
     where nothing may be read, TV_E_HALO and untouched arrays where a needed plane is missing;
  3. slabs whose halos are the neighbouring slab's own arrays (ADMM: a SPARSELY stored t') give the unsharded call; tv_cheb_step and
     the kernel-pair entry points (tv_cp_dual, tv_cp_primal, tv_admm_zu, tv_admm_tu, tv_DT_axpy, tv_DT_axpy2) on the same slabs;
  4. empty ranges, ranges outside the slab, one-plane slabs.

The reference is NumPy in float64 over the oracle's D / D^T: one iteration written out.  Every tolerance is one the suite already
uses for the same quantity (test_admm_fused_calls_match_numpy, test_cp_operator_one_sweep_equals_kernel_pair_and_oracle,
test_slab_calls_equal_unsharded) or exact equality.

A property of the design (include/pytv4d.h, at tv_cp_fixup): x_out / r of a site next to a z-seam is rounded once by the sweep and once
more by the fix-up, a site inside a chunk once only.  Slabs reproduce the unsharded arrays bit for bit when their cuts fall on the
unsharded call's chunk seams (multiples of tv_cp_zchunk); other cuts move seams, and x_out / r then agree to the rounding of the
dtype only -- those are held to the float64 reference at the tolerances of part 1, while q, u and the stored samples of t'
(site-local arithmetic) stay bit-identical.  Measured (profiles/r8_sweep_ranges_tests.txt): off the seams x_out / r differed in 240 of
240 combinations, on the seams in none; run with -s to see the verdict per array."""
import os

import numpy as np
import pytest

from conftest import SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

os.environ["TV_MARCH_MIN_PLANE_KB"] = "0"
os.environ["TV_FUSED_MIN_KVOXELS"] = "0"

KW = dict(reg_z_over_reg=1.3, reg_time=0.6)
THRESH, RHO = 0.7, 0.15                                   # ADMM (test_admm_fused_calls_match_numpy)
LAM, SIGMA_D, SIGMA_A, TAU = 5.0, 0.5, 1.0, 0.05          # Chambolle-Pock
SENT = 7.0                                                # what output arrays hold before a call
E_ARG, E_HALO = -1, -2
FID_OF_INPUT, FID_BOTH = 1, 2

# the smallest shapes at which each seam exists (the one-sweep path needs nx >= 64)
CASES = [((7, 3, 10, 64), np.float32),       # one block tile; ny ragged against the 8-row wave tile
         ((7, 3, 10, 64), np.float64),
         ((6, 2, 9, 320), np.float32),       # crosses the 256-column block tile, a partial tile follows
         ((5, 9, 5, 68), np.float32),        # M > 8: one time-window seam; partial wave tile
         ((5, 9, 5, 66), np.float64),        # the same in fp64 (2 columns per lane)
         ((4, 1, 8, 64), np.float32)]        # M = 1, no time axis
SLAB_CASES = [c for c in CASES if c[0][0] in (7, 5)]
CASE_IDS = ["%s-%s" % ("x".join(map(str, s)), np.dtype(d).name) for s, d in CASES]
SLAB_IDS = ["%s-%s" % ("x".join(map(str, s)), np.dtype(d).name) for s, d in SLAB_CASES]

# (kind, option, separate output array for the dual variable): option = flags of tv_cp_sweep / full_store of tv_admm_sweep.
# ("cp", 0, False) goes through tv_cp_fused, ("admm", f, False) through tv_admm_fused
CP_VARIANTS = [("cp", f, pp) for f in (0, FID_OF_INPUT, FID_OF_INPUT | FID_BOTH) for pp in (False, True)]
ADMM_VARIANTS = [("admm", f, True) for f in (0, 1, 2, 3)] + [("admm", 0, False)]
ALL_VARIANTS = CP_VARIANTS + ADMM_VARIANTS + [("cpop", 0, False)]
FEW_VARIANTS = [("cp", 0, False), ("cp", FID_OF_INPUT | FID_BOTH, True), ("admm", 0, True), ("cpop", 0, False)]


@pytest.fixture(scope="module")
def nvlib():
    import pytv  # noqa: F401
    from pytv import _native as nv
    return nv


def _tols(dtype):
    """ADMM: tol of test_admm_fused_calls_match_numpy; CP: rtol, atol of x, atol of q and p."""
    if dtype == np.float64:
        return dict(tol=1e-11, rtol=1e-10, atol_x=1e-9, atol_q=1e-10)
    return dict(tol=3e-5, rtol=1e-5, atol_x=1e-3, atol_q=1e-4)


# ------------------------------------------------------------------------------------------------
# inputs and the float64 reference of one iteration: computed once per (scheme, shape, dtype), never modified
# ------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, scheme, shape, dtype):
        self.scheme, self.shape, self.dtype = scheme, tuple(shape), dtype
        rng = np.random.default_rng(17)
        f8 = np.float64
        # ADMM: v = D x + u; z = shrink(v); u' = v - z; t' = (z - u') - D x; r = (x0 - x) + rho D^T t'
        self.ax = (rng.random(shape) * 4).astype(dtype)
        self.ax0 = (self.ax + rng.random(shape)).astype(dtype)
        dx = orc.D(self.ax.astype(f8), scheme, **KW)
        self.nd = dx.shape[1]
        self.au = rng.standard_normal(dx.shape).astype(dtype)
        v = dx + self.au.astype(f8)
        nv_ = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            z = v * np.where(nv_ > 0, np.maximum(0.0, 1.0 - THRESH / nv_), 0.0)
        assert (nv_ > THRESH).any()                                             # the shrinkage is active (a condition on the input)
        self.a_un = v - z
        self.a_t = (z - self.a_un) - dx
        self.a_r = (self.ax0.astype(f8) - self.ax) + RHO * orc.D_T(self.a_t, scheme, **KW)
        self.a_tv = float(orc.compute_L21_norm(dx))
        self.a_rr = float(np.sum(self.a_r * self.a_r))
        self.a_fid = float(np.sum((self.ax.astype(f8) - self.ax0.astype(f8)) ** 2))
        self.a_z = z
        # Chambolle-Pock: q' = proj(q + sigma D x); p' = (p + sigma_A (x - x0)) / (1 + sigma_A); x' = x - tau p' - tau D^T q'
        self.cx0 = (50.0 * rng.random(shape)).astype(dtype)
        self.cx = (25.0 + rng.standard_normal(shape)).astype(dtype)
        self.cq = (LAM / np.sqrt(self.nd) * rng.standard_normal(dx.shape)).astype(dtype)     # |q| scatters around lambda
        self.cp = rng.standard_normal(shape).astype(dtype)
        x, x0, p = self.cx.astype(f8), self.cx0.astype(f8), self.cp.astype(f8)
        dxc = orc.D(x, scheme, **KW)
        v = self.cq.astype(f8) + SIGMA_D * dxc
        nrm = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        assert (nrm > LAM).mean() > 0.1 and (nrm < LAM).mean() > 0.1             # both branches of the projection (a condition on the input)
        self.c_qn = v / np.maximum(1.0, nrm / LAM)
        self.c_pn = (p + SIGMA_A * (x - x0)) / (1.0 + SIGMA_A)
        dtq = orc.D_T(self.c_qn, scheme, **KW)
        self.c_xo = x - TAU * self.c_pn - TAU * dtq
        self.o_xo = x - TAU * p - TAU * dtq                                       # tv_cpop_fused with A^T p = p
        self.c_tv = float(orc.compute_L21_norm(dxc))
        self.c_fid_in = 0.5 * float(np.sum((x - x0) ** 2))
        self.c_fid_out = 0.5 * float(np.sum((self.c_xo - x0) ** 2))
        self._dev = {}

    def dev(self, name):
        """read-only device master of an input array (callers clone what a kernel writes)"""
        import torch
        if name not in self._dev:
            self._dev[name] = torch.as_tensor(getattr(self, name)).cuda()
        return self._dev[name]


_PROBLEMS = {}


def problem(scheme, shape, dtype):
    key = (scheme, tuple(shape), np.dtype(dtype).name)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(scheme, shape, dtype)
    return _PROBLEMS[key]


def z_channels(scheme):
    """(ch_back, ch_fwd): the z channel whose adjoint looks backwards / forwards -- the planes tv_DT names y_prev / y_next"""
    per = 2 if scheme == "hybrid" else 1
    return 2 * per, 2 * per + (1 if scheme == "hybrid" else 0)


# ------------------------------------------------------------------------------------------------
# one algorithm variant: device state of a slab, the sweep call, the fix-up call
# ------------------------------------------------------------------------------------------------
class Alg:
    def __init__(self, nv, variant):
        self.nv, self.lib = nv, nv.lib()
        self.kind, self.opt, self.sep = variant
        self.outputs = {"cp": ("xo", "qo", "p"), "admm": ("r", "uo", "t"), "cpop": ("xo", "q")}[self.kind]

    def x_master(self, P):
        return P.dev("ax" if self.kind == "admm" else "cx")

    def state(self, P, a=0, b=None):
        """fresh device arrays for the planes [a, b): inputs copied, outputs filled with SENT"""
        import torch
        b = P.shape[0] if b is None else b
        s = {}
        if self.kind == "admm":
            s["x"], s["x0"], s["u"] = P.dev("ax")[a:b], P.dev("ax0")[a:b], P.dev("au")[a:b].clone()
            s["uo"] = torch.full_like(s["u"], SENT) if self.sep else s["u"]
            s["t"], s["r"] = torch.full_like(s["u"], SENT), torch.full_like(s["x"], SENT)
        else:
            s["x"], s["q"] = P.dev("cx")[a:b], P.dev("cq")[a:b].clone()
            s["p"] = P.dev("cp")[a:b].clone()
            s["xo"] = torch.full_like(s["x"], SENT)
            if self.kind == "cp":
                s["x0"] = P.dev("cx0")[a:b]
                s["qo"] = torch.full_like(s["q"], SENT) if self.sep else s["q"]
        return s

    def halo_src(self, s):
        """the array whose boundary planes are the neighbouring slab's q_prev / q_next (t_prev / t_next)"""
        return s[{"cp": "qo", "admm": "t", "cpop": "q"}[self.kind]]

    def sweep(self, g, s, xp, xn, cb, cc, sc):
        """sc: three fp64 words (tv, second partial, third partial under TV_CP_FID_BOTH); returns the status"""
        nv, lib = self.nv, self.lib
        ptr, st, ws = nv.ptr, nv.current_stream(s["x"].device), nv.ptr(g.workspace())
        tvp, fp = sc[0:1].data_ptr(), sc[1:3].data_ptr()
        if self.kind == "cp":
            if self.opt == 0 and not self.sep:
                return lib.tv_cp_fused(g.ref, ptr(s["x"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["x0"]), ptr(s["p"]), ptr(s["xo"]), SIGMA_D, LAM,
                                       TAU, SIGMA_A, cb, cc, tvp, fp, ws, st)
            return lib.tv_cp_sweep(g.ref, ptr(s["x"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["qo"]), ptr(s["x0"]), ptr(s["p"]), ptr(s["xo"]),
                                   SIGMA_D, LAM, TAU, SIGMA_A, self.opt, cb, cc, tvp, fp, ws, st)
        if self.kind == "admm":
            if not self.sep:
                return lib.tv_admm_fused(g.ref, ptr(s["x"]), ptr(xp), ptr(xn), ptr(s["u"]), ptr(s["t"]), ptr(s["x0"]), ptr(s["r"]), THRESH, RHO,
                                         self.opt, cb, cc, tvp, fp, ws, st)
            return lib.tv_admm_sweep(g.ref, ptr(s["x"]), ptr(xp), ptr(xn), ptr(s["u"]), ptr(s["uo"]), ptr(s["t"]), ptr(s["x0"]), ptr(s["r"]),
                                     THRESH, RHO, self.opt, cb, cc, tvp, fp, ws, st)
        return lib.tv_cpop_fused(g.ref, ptr(s["x"]), ptr(xp), ptr(xn), ptr(s["q"]), ptr(s["p"]), ptr(s["xo"]), SIGMA_D, LAM, TAU, cb, cc, tvp, ws, st)

    def fixup(self, g, s, hp, hn, zb, zc, sc):
        """sc: one fp64 word (tv_cpop_fixup returns no scalar: the word stays as it was)"""
        nv, lib = self.nv, self.lib
        ptr, st, ws = nv.ptr, nv.current_stream(s["x"].device), nv.ptr(g.workspace())
        if self.kind == "cp":
            x0 = None if self.opt == FID_OF_INPUT else s["x0"]                       # lagged fidelity alone: the fix-up needs no x0
            return lib.tv_cp_fixup(g.ref, ptr(s["qo"]), ptr(hp), ptr(hn), ptr(s["xo"]), ptr(x0), TAU, zb, zc, sc.data_ptr(), ws, st)
        if self.kind == "admm":
            return lib.tv_admm_fixup(g.ref, ptr(s["t"]), ptr(hp), ptr(hn), ptr(s["r"]), RHO, zb, zc, sc.data_ptr(), ws, st)
        return lib.tv_cpop_fixup(g.ref, ptr(s["q"]), ptr(hp), ptr(hn), ptr(s["xo"]), TAU, zb, zc, ws, st)

    @property
    def fix_scalar_defined(self):
        """tv_cpop_fixup has none; tv_admm_fixup's is meaningless after a sweep with full_store bit 1"""
        return self.kind == "cp" or (self.kind == "admm" and not (self.opt & 2))

    def out(self, s):
        return {k: s[k] for k in self.outputs}

    def check_reference(self, P, o, sw, fx, what=""):
        """outputs o (name -> tensor), summed sweep scalars sw[3] and fix-up scalar fx against the float64 iteration"""
        T = _tols(P.dtype)
        tol, rtol = T["tol"], T["rtol"]
        n = {k: v.cpu().numpy() for k, v in o.items()}
        msg = "%s %s %s %s %s" % (self.kind, self.opt, P.scheme, P.shape, what)
        if self.kind == "admm":
            scale = max(1.0, np.abs(P.a_r).max())
            np.testing.assert_allclose(n["uo"], P.a_un, rtol=0, atol=tol * 10, err_msg="u " + msg)
            np.testing.assert_allclose(n["r"], P.a_r, rtol=0, atol=tol * 10 * scale, err_msg="r " + msg)
            np.testing.assert_allclose(sw[0], P.a_tv, rtol=max(tol, 1e-12) * 10, err_msg="tv " + msg)
            if self.opt & 2:
                np.testing.assert_allclose(sw[1], P.a_fid, rtol=max(tol, 1e-12) * 10, err_msg="|x - x0|^2 " + msg)
            else:
                np.testing.assert_allclose(sw[1] + fx, P.a_rr, rtol=tol * 100, err_msg="<r, r> " + msg)
            stored = np.ones(n["t"].shape, bool) if (self.opt & 1) else (n["t"] != SENT)
            assert stored.any()
            np.testing.assert_allclose(n["t"][stored], P.a_t[stored], rtol=0, atol=tol * 10, err_msg="t' " + msg)
            return
        want_x = P.c_xo if self.kind == "cp" else P.o_xo
        np.testing.assert_allclose(n["xo"], want_x, rtol=rtol, atol=T["atol_x"], err_msg="x " + msg)
        np.testing.assert_allclose(n["qo" if self.kind == "cp" else "q"], P.c_qn, rtol=rtol, atol=T["atol_q"], err_msg="q " + msg)
        np.testing.assert_allclose(sw[0], P.c_tv, rtol=rtol, err_msg="tv " + msg)
        if self.kind == "cp":
            np.testing.assert_allclose(n["p"], P.c_pn, rtol=rtol, atol=T["atol_q"], err_msg="p " + msg)
            if self.opt == 0:
                np.testing.assert_allclose(sw[1] + fx, P.c_fid_out, rtol=rtol, err_msg="fid " + msg)
            else:
                np.testing.assert_allclose(sw[1], P.c_fid_in, rtol=rtol, err_msg="fid of the input " + msg)
                if self.opt & FID_BOTH:
                    np.testing.assert_allclose(sw[2] + fx, P.c_fid_out, rtol=rtol, err_msg="fid of the output " + msg)
                else:
                    assert fx == 0.0


def _geom(nv, P, nz=None, nz_global=None, z0=0):
    import torch
    shape = P.shape if nz is None else (nz,) + P.shape[1:]
    return nv.Geometry(shape, P.scheme, torch.as_tensor(P.ax).dtype, torch.device("cuda", 0), nz_global=nz_global, z0=z0, **KW)


def _scalars(n, width, fill=0.0):
    import torch
    return torch.full((max(n, 1), width), fill, dtype=torch.float64, device="cuda")


def run_ranges(nv, alg, g, s, chunk_ranges, plane_ranges, xh=(None, None), qh=(None, None)):
    """the sweep over each chunk range, then the fix-up over each plane range, every call with scalar slots of its own;
    returns the summed sweep scalars [3] and the summed fix-up scalar"""
    sw, fx = _scalars(len(chunk_ranges), 3), _scalars(len(plane_ranges), 1)
    for i, (cb, cc) in enumerate(chunk_ranges):
        nv.check(alg.sweep(g, s, xh[0], xh[1], cb, cc, sw[i]))
    for i, (zb, zn) in enumerate(plane_ranges):
        nv.check(alg.fixup(g, s, qh[0], qh[1], zb, zn, fx[i]))
    return sw.sum(dim=0).cpu().numpy(), float(fx.sum())


def _close12(a, b):
    """summed fp64 partials against the whole call's scalar: the bound of test_slab_calls_equal_unsharded"""
    return abs(a - b) <= 1e-12 * abs(b)


def chunk_partitions(nch):
    parts = [[(k, 1) for k in reversed(range(nch))]]                         # every chunk on its own, in reverse order
    if nch >= 2:
        na = (nch - 2 + 1) // 2
        nb = nch - 2 - na
        parts.append([(1, na), (0, 1), (nch - 1, 1), (1 + na, nb)])          # the solver's interior-first order
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


def test_partitions_cover_every_chunk_and_plane_once():
    """the helpers above (no GPU work): every list is a partition, the mid-chunk split exists at the shapes of this file"""
    for nch in range(1, 6):
        for part in chunk_partitions(nch):
            assert sorted(k for b, c in part for k in range(b, b + c)) == list(range(nch))
    for nz in (4, 5, 6, 7):
        for zc in (2, 3):
            parts = plane_partitions(nz, zc)
            assert len(parts) == 3 and parts[2][0][0] % zc != 0
            for part in parts:
                assert sorted(k for b, c in part for k in range(b, b + c)) == list(range(nz))


# ------------------------------------------------------------------------------------------------
# 1. range partition invariance (unsharded, no halos)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_chunk_and_plane_ranges_equal_the_whole_call(nvlib, scheme, case, zchunk, tvopt):
    """Every sweep variant as ONE call (against the float64 iteration), then on fresh copies of the inputs as separate calls over a
    partition of the chunks followed by the fix-up over a partition of the planes: every output array -- the sentinel-filled
    samples of a sparsely stored t' included -- bit-identical to the whole call, the partial scalars summing to its scalars."""
    import torch
    nv = nvlib
    tvopt("TV_ZCHUNK", zchunk)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    g = _geom(nv, P)
    assert nv.lib().tv_cp_fused_supported(g.ref) == 1
    nz, zc = shape[0], nv.lib().tv_cp_zchunk(g.ref)
    assert zc == min(int(zchunk), nz)
    nch = (nz + zc - 1) // zc
    cparts, pparts = chunk_partitions(nch), plane_partitions(nz, zc)
    assert len(cparts) == 3 and len(pparts) == 3
    for variant in ALL_VARIANTS:
        alg = Alg(nv, variant)
        s0 = alg.state(P)
        sw0, fx0 = run_ranges(nv, alg, g, s0, [(0, -1)], [(0, -1)])
        alg.check_reference(P, alg.out(s0), sw0, fx0, "whole call, TV_ZCHUNK=%s" % zchunk)
        for cpart, ppart in zip(cparts, pparts):
            s1 = alg.state(P)
            sw1, fx1 = run_ranges(nv, alg, g, s1, cpart, ppart)
            for k in alg.outputs:
                assert torch.equal(s1[k], s0[k]), (variant, k, cpart, ppart, _first_difference(s1[k], s0[k]))
            assert _close12(sw1[0], sw0[0]) and _close12(sw1[1], sw0[1]) and _close12(sw1[2], sw0[2]), (variant, cpart, sw1, sw0)
            if alg.fix_scalar_defined:
                assert _close12(fx1, fx0), (variant, ppart, fx1, fx0)


def _first_difference(a, b):
    """index (plane first) and values of the first element in which two arrays differ: what an assertion message shows"""
    import torch
    d = torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b))))
    if d.numel() == 0:
        return None
    i = tuple(int(v) for v in d[0])
    return i, float(a[i]), float(b[i]), int(d.shape[0])


# ------------------------------------------------------------------------------------------------
# 2. who reads which halo
# ------------------------------------------------------------------------------------------------
def _same(alg, sa, sb, *scalars):
    import torch
    for k in alg.outputs:
        if not torch.equal(sa[k], sb[k]):
            return False
    return all(torch.equal(a, b) for a, b in zip(scalars[0::2], scalars[1::2]))


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_only_the_edge_chunks_and_planes_read_the_halos(nvlib, scheme, case, zchunk, tvopt):
    """A slab in the middle of a volume (z0 = 2, nz_global = nz + 4).  Interior chunks / planes run without halo pointers and give the
    same bits next to NaN halos; the first chunk ignores x_next, the last x_prev, plane 0 ignores q_next, plane nz-1 q_prev.  A range
    that touches the slab edge without the halo its scheme reads there is refused with TV_E_HALO before anything is written."""
    import torch
    nv = nvlib
    tvopt("TV_ZCHUNK", zchunk)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    nz = shape[0]
    g = _geom(nv, P, nz_global=nz + 4, z0=2)
    zc = nv.lib().tv_cp_zchunk(g.ref)
    nch = (nz + zc - 1) // zc
    assert nch >= 2
    rng = np.random.default_rng(23)
    tdt = torch.as_tensor(P.ax).dtype

    def plane(fill=None):
        if fill is None:
            return torch.as_tensor(rng.standard_normal(shape[1:]).astype(dtype)).cuda()
        return torch.full(shape[1:], fill, dtype=tdt, device="cuda")
    xp, xn, hp, hn, nan = plane(), plane(), plane(), plane(), plane(float("nan"))
    # the halo a scheme reads: forward differences need x(z+1) and the adjoint's y(z-1), backward ones the opposite
    x_prev_read, x_next_read = scheme != "upwind", scheme != "downwind"
    q_prev_read, q_next_read = scheme != "downwind", scheme != "upwind"
    for variant in FEW_VARIANTS:
        alg = Alg(nv, variant)

        def sweep(rng_, a, b):
            s, sc = alg.state(P), _scalars(1, 3, 123.0)
            rc = alg.sweep(g, s, a, b, rng_[0], rng_[1], sc[0])
            return rc, s, sc

        interior = (1, max(nch - 2, 0))
        for rng_, good, bad in ((interior, (None, None), (nan, nan)), ((0, 1), (xp, xn), (xp, nan)), ((nch - 1, 1), (xp, xn), (nan, xn))):
            rc_a, s_a, sc_a = sweep(rng_, *good)
            rc_b, s_b, sc_b = sweep(rng_, *bad)
            assert rc_a == 0 and rc_b == 0, (variant, rng_, nv.lib().tv_last_error())
            assert _same(alg, s_a, s_b, sc_a, sc_b), (variant, "sweep", rng_)
            assert bool(torch.isfinite(sc_a).all())
        # the halo is really read where it should be: another x_prev / x_next changes the edge chunk
        if x_prev_read:
            assert not _same(alg, sweep((0, 1), xp, xn)[1], sweep((0, 1), xn, xn)[1]), (variant, "x_prev unused")
        if x_next_read:
            assert not _same(alg, sweep((nch - 1, 1), xp, xn)[1], sweep((nch - 1, 1), xp, xp)[1]), (variant, "x_next unused")
        # missing halos
        for rng_, halos, needed in (((0, 1), (None, xn), x_prev_read), ((nch - 1, 1), (xp, None), x_next_read), ((0, -1), (None, None), True)):
            s, sc = alg.state(P), _scalars(1, 3, 123.0)
            before = {k: v.clone() for k, v in s.items()}
            rc = alg.sweep(g, s, halos[0], halos[1], rng_[0], rng_[1], sc[0])
            if needed:
                assert rc == E_HALO, (variant, rng_, rc)
                assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), (variant, rng_, "written to")
            else:
                assert rc == 0, (variant, rng_, rc)

        def fix(rng_, a, b):
            s = alg.state(P)
            sw = _scalars(1, 3)
            nv.check(alg.sweep(g, s, xp, xn, 0, -1, sw[0]))
            before = {k: v.clone() for k, v in s.items()}
            sc = _scalars(1, 1, 123.0)
            rc = alg.fixup(g, s, a, b, rng_[0], rng_[1], sc[0])
            return rc, s, sc, before

        for rng_, good, bad in (((1, nz - 2), (None, None), (nan, nan)), ((0, 1), (hp, hn), (hp, nan)), ((nz - 1, 1), (hp, hn), (nan, hn))):
            rc_a, s_a, sc_a, _ = fix(rng_, *good)
            rc_b, s_b, sc_b, _ = fix(rng_, *bad)
            assert rc_a == 0 and rc_b == 0, (variant, rng_, nv.lib().tv_last_error())
            assert _same(alg, s_a, s_b, sc_a, sc_b), (variant, "fix-up", rng_)
            assert bool(torch.isfinite(sc_a).all())
        if q_prev_read:
            assert not _same(alg, fix((0, 1), hp, hn)[1], fix((0, 1), hn, hn)[1]), (variant, "q_prev unused")
        if q_next_read:
            assert not _same(alg, fix((nz - 1, 1), hp, hn)[1], fix((nz - 1, 1), hp, hp)[1]), (variant, "q_next unused")
        for rng_, halos, needed in (((0, 1), (None, hn), q_prev_read), ((nz - 1, 1), (hp, None), q_next_read), ((0, -1), (None, None), True)):
            rc, s, sc, before = fix(rng_, *halos)
            if needed:
                assert rc == E_HALO, (variant, rng_, rc)
                assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), (variant, rng_, "written to")
            else:
                assert rc == 0, (variant, rng_, rc)


# ------------------------------------------------------------------------------------------------
# 3. slabs equal the unsharded call, in-process
# ------------------------------------------------------------------------------------------------
def run_slabs(nv, alg, P, cuts):
    """every slab swept with x halos out of the neighbouring slabs, then every slab fixed up with the boundary plane of the
    neighbour's q_out / t' in the channel tv_DT names for that side; returns the concatenated outputs and the summed scalars"""
    import torch
    nzg = P.shape[0]
    X = alg.x_master(P)
    ch_back, ch_fwd = z_channels(P.scheme)
    slabs = list(zip(cuts[:-1], cuts[1:]))
    geoms = [_geom(nv, P, nz=b - a, nz_global=nzg, z0=a) for a, b in slabs]
    states = [alg.state(P, a, b) for a, b in slabs]
    sw, fx = _scalars(len(slabs), 3), _scalars(len(slabs), 1)
    for i, (a, b) in enumerate(slabs):
        xp = X[a - 1].clone() if a > 0 else None
        xn = X[b].clone() if b < nzg else None
        nv.check(alg.sweep(geoms[i], states[i], xp, xn, 0, -1, sw[i]))
    for i, (a, b) in enumerate(slabs):
        hp = alg.halo_src(states[i - 1])[-1, ch_back].clone() if a > 0 else None
        hn = alg.halo_src(states[i + 1])[0, ch_fwd].clone() if b < nzg else None
        nv.check(alg.fixup(geoms[i], states[i], hp, hn, 0, -1, fx[i]))
    out = {k: torch.cat([s[k] for s in states]) for k in alg.outputs}
    return out, sw.sum(dim=0).cpu().numpy(), float(fx.sum())


def check_slabs(nv, alg, P, cuts, zc_whole, whole):
    """slab outputs against the unsharded call `whole` = (outputs, sw, fx) -- bit for bit when the cuts fall on its chunk seams (module
    docstring), else q / u / stored t' bit for bit and x_out / r against the float64 reference -- or, whole = None, the reference alone"""
    import torch
    out, sw, fx = run_slabs(nv, alg, P, cuts)
    if whole is None:
        alg.check_reference(P, out, sw, fx, "slabs %s" % (cuts,))
        return
    o0, sw0, fx0 = whole
    aligned = all(c % zc_whole == 0 for c in cuts[1:-1])
    assert _close12(sw[0], sw0[0]), (alg.kind, alg.opt, cuts, "tv", sw[0], sw0[0])
    if aligned:
        for k in alg.outputs:
            assert torch.equal(out[k], o0[k]), (alg.kind, alg.opt, k, cuts, _first_difference(out[k], o0[k]))
        assert _close12(sw[1], sw0[1]) and _close12(sw[2], sw0[2]), (alg.kind, alg.opt, cuts, sw, sw0)
        if alg.fix_scalar_defined:
            assert _close12(fx, fx0), (alg.kind, alg.opt, cuts, fx, fx0)
        return
    for k in alg.outputs:
        same = torch.equal(out[k], o0[k])
        print("slabs %s zc=%d %s/%s %s %s %s: %s" % (cuts, zc_whole, alg.kind, alg.opt, P.scheme, P.shape, k, "bit-identical" if same else "differs"))
        if k in ("qo", "q", "uo", "p"):                                     # site-local arithmetic: no seam enters
            assert same, (alg.kind, alg.opt, k, cuts, _first_difference(out[k], o0[k]))
        elif k == "t":                                                      # other seams, other stored samples; the common ones agree
            both = (out[k] != SENT) & (o0[k] != SENT)
            assert bool(both.any()) and torch.equal(out[k][both], o0[k][both]), (alg.kind, alg.opt, k, cuts)
    alg.check_reference(P, out, sw, fx, "slabs %s" % (cuts,))


SLAB_VARIANTS = [("cp", 0, False), ("cp", FID_OF_INPUT | FID_BOTH, True), ("admm", 0, True), ("admm", 2, True), ("cpop", 0, False)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", SLAB_CASES, ids=SLAB_IDS)
@pytest.mark.parametrize("zchunk", ["2", "3"])
def test_slabs_with_their_neighbours_arrays_as_halos_equal_unsharded(nvlib, scheme, case, zchunk, tvopt):
    """Cuts (0, 3, nz), one-plane slabs, and cuts on the chunk seams.  ADMM runs with full_store bit 0 clear: the t' halo plane comes
    out of a SPARSELY stored neighbour, the promise of the header's "the samples ... the neighbouring ranks read"."""
    nv = nvlib
    tvopt("TV_ZCHUNK", zchunk)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    nz = shape[0]
    g = _geom(nv, P)
    zc = nv.lib().tv_cp_zchunk(g.ref)
    cut_sets = [(0, 3, nz), tuple(range(nz + 1)), tuple(range(0, nz, zc)) + (nz,)]
    for variant in SLAB_VARIANTS:
        alg = Alg(nv, variant)
        s0 = alg.state(P)
        sw0, fx0 = run_ranges(nv, alg, g, s0, [(0, -1)], [(0, -1)])
        for cuts in cut_sets:
            check_slabs(nv, alg, P, cuts, zc, (alg.out(s0), sw0, fx0))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_slabs_with_the_librarys_own_chunk_lengths_match_the_reference(nvlib, scheme, tvopt):
    """TV_ZCHUNK not set (0): the library chooses other chunk lengths for a slab than for the whole volume -- the float64 reference only."""
    nv = nvlib
    tvopt("TV_ZCHUNK", 0)
    for shape, dtype in SLAB_CASES[:3]:
        P = problem(scheme, shape, dtype)
        nz = shape[0]
        lens = {nv.lib().tv_cp_zchunk(_geom(nv, P, nz=b - a, nz_global=nz, z0=a).ref) for a, b in ((0, 3), (3, nz))}
        assert lens != {nv.lib().tv_cp_zchunk(_geom(nv, P).ref)}
        for variant in SLAB_VARIANTS:
            for cuts in ((0, 3, nz), tuple(range(nz + 1))):
                check_slabs(nv, Alg(nv, variant), P, cuts, 0, None)


def _two_planes(x, lo):
    """two-plane halo (lo, lo + 1) of x, NaN where the global plane does not exist (must never be read)"""
    import torch
    buf = torch.full((2,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype, device=x.device)
    for k in range(2):
        if 0 <= lo + k < x.shape[0]:
            buf[k] = x[lo + k]
    return buf


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", SLAB_CASES + [((7, 3, 8, 12), np.float64)], ids=SLAB_IDS + ["7x3x8x12-float64"])
def test_cheb_step_and_kernel_pairs_on_slabs_equal_unsharded(nvlib, scheme, case, tvopt):
    """tv_cheb_step (two-plane halos; with and without y, add, ref; dots = NULL) held to the standard of
    test_normal_op2_on_slabs_equals_unsharded -- the output bit for bit, the summed dots to 1e-12 -- and the kernel-pair entry points
    with one-plane halos: every output array bit for bit, summed scalars to 1e-12.  (7, 3, 8, 12) takes the one-site kernels."""
    import torch
    nv, lib = nvlib, nvlib.lib()
    tvopt("TV_ZCHUNK", 2)
    shape, dtype = case
    P = problem(scheme, shape, dtype)
    nz = shape[0]
    ch_back, ch_fwd = z_channels(scheme)
    rng = np.random.default_rng(29)
    x, x0, u, q, p, xc = P.dev("ax"), P.dev("ax0"), P.dev("au"), P.dev("cq"), P.dev("cp"), P.dev("cx")
    bvec, yvec, add, ref = [torch.as_tensor((rng.standard_normal(shape) * 3).astype(dtype)).cuda() for _ in range(4)]
    ab = q - u                                                             # the halo planes of tv_DT_axpy(a, b) hold a - b
    st = nv.current_stream(x.device)
    alpha, beta = 0.8, 0.3
    cheb_modes = ((True, 0.0, True, True), (False, 0.0, False, False), (True, 0.0, False, False), (False, 0.4, False, True))

    def calls(g, a, b):
        """every entry point on the planes [a, b) of the volume; returns name -> (arrays, scalars)"""
        ws, res = nv.ptr(g.workspace()), {}
        sl = slice(a, b)
        first, last = a == 0, b == nz
        xp1, xn1 = (None if first else x[a - 1].clone()), (None if last else x[b].clone())
        xp2, xn2 = (None if first else _two_planes(x, a - 2)), (None if last else _two_planes(x, b))
        qp, qn = (None if first else q[a - 1, ch_back].clone()), (None if last else q[b, ch_fwd].clone())
        abp, abn = (None if first else ab[a - 1, ch_back].clone()), (None if last else ab[b, ch_fwd].clone())
        for i, (use_y, yscale, use_add, use_ref) in enumerate(cheb_modes):
            o, dots = torch.full_like(x[sl], SENT), torch.zeros(2, dtype=torch.float64, device="cuda")
            args = (g.ref, nv.ptr(x[sl]), nv.ptr(xp2), nv.ptr(xn2), RHO, nv.ptr(bvec[sl]), nv.ptr(yvec[sl]) if use_y else None, yscale,
                    nv.ptr(add[sl]) if use_add else None, nv.ptr(ref[sl]) if use_ref else None, alpha, beta)
            nv.check(lib.tv_cheb_step(*args, nv.ptr(o), dots.data_ptr(), ws, st))
            res["cheb%d" % i] = ([o], dots)
            if not use_ref:                                                # dots = NULL: the same output, no dot products (ref needs dots)
                o2 = torch.full_like(x[sl], SENT)
                nv.check(lib.tv_cheb_step(*args, nv.ptr(o2), None, ws, st))
                assert torch.equal(o2, o), ("dots = NULL", i, a, b)
        sc = torch.zeros(4, dtype=torch.float64, device="cuda")
        qd = q[sl].clone()
        xcp, xcn = (None if first else xc[a - 1].clone()), (None if last else xc[b].clone())
        nv.check(lib.tv_cp_dual(g.ref, nv.ptr(xc[sl]), nv.ptr(xcp), nv.ptr(xcn), nv.ptr(qd), SIGMA_D, LAM, sc[0:1].data_ptr(), ws, st))
        res["cp_dual"] = ([qd], sc[0:1])
        xq, pq = x[sl].clone(), p[sl].clone()
        nv.check(lib.tv_cp_primal(g.ref, nv.ptr(q[sl]), nv.ptr(qp), nv.ptr(qn), nv.ptr(xq), nv.ptr(x0[sl]), nv.ptr(pq), TAU, SIGMA_A,
                                  sc[1:2].data_ptr(), ws, st))
        res["cp_primal"] = ([xq, pq], sc[1:2])
        for name, k in (("tv_admm_zu", 2), ("tv_admm_tu", 3)):
            zz, uu = torch.full_like(u[sl], SENT), u[sl].clone()
            nv.check(getattr(lib, name)(g.ref, nv.ptr(x[sl]), nv.ptr(xp1), nv.ptr(xn1), nv.ptr(zz), nv.ptr(uu), THRESH, sc[k:k + 1].data_ptr(), ws, st))
            res[name] = ([zz, uu], sc[k:k + 1])
        o1, o2 = torch.full_like(x[sl], SENT), torch.full_like(x[sl], SENT)
        nv.check(lib.tv_DT_axpy(g.ref, nv.ptr(q[sl]), nv.ptr(u[sl]), nv.ptr(abp), nv.ptr(abn), nv.ptr(x0[sl]), RHO, nv.ptr(o1), st))
        nv.check(lib.tv_DT_axpy2(g.ref, nv.ptr(q[sl]), nv.ptr(u[sl]), nv.ptr(abp), nv.ptr(abn), nv.ptr(x[sl]), nv.ptr(p[sl]), -TAU, -TAU, nv.ptr(o2), st))
        res["DT_axpy"] = ([o1, o2], sc[0:0])
        return res

    whole = calls(_geom(nv, P), 0, nz)
    for cuts in ((0, 3, nz), tuple(range(nz + 1))):
        parts = [calls(_geom(nv, P, nz=b - a, nz_global=nz, z0=a), a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        for name, (arrs, sc) in whole.items():
            for k, arr in enumerate(arrs):
                got = torch.cat([pt[name][0][k] for pt in parts])
                assert torch.equal(got, arr), (name, k, cuts, _first_difference(got, arr))
            if sc.numel():
                tot = sum(pt[name][1].cpu().numpy() for pt in parts)
                np.testing.assert_allclose(tot, sc.cpu().numpy(), rtol=1e-12, err_msg="%s %s" % (name, cuts))
    # the unsharded calls themselves against the float64 reference (tolerances of part 1)
    T = _tols(dtype)
    f8 = np.float64
    np.testing.assert_allclose(whole["cp_dual"][0][0].cpu().numpy(), P.c_qn, rtol=T["rtol"], atol=T["atol_q"])
    np.testing.assert_allclose(float(whole["cp_dual"][1]), P.c_tv, rtol=T["rtol"])
    np.testing.assert_allclose(whole["tv_admm_zu"][0][0].cpu().numpy(), P.a_z, rtol=0, atol=T["tol"] * 10)
    np.testing.assert_allclose(whole["tv_admm_zu"][0][1].cpu().numpy(), P.a_un, rtol=0, atol=T["tol"] * 10)
    np.testing.assert_allclose(whole["tv_admm_tu"][0][0].cpu().numpy(), P.a_z - P.a_un, rtol=0, atol=T["tol"] * 10)
    want = P.ax0.astype(f8) + RHO * orc.D_T(P.cq.astype(f8) - P.au.astype(f8), scheme, **KW)
    np.testing.assert_allclose(whole["DT_axpy"][0][0].cpu().numpy(), want, rtol=T["rtol"], atol=T["atol_x"])


# ------------------------------------------------------------------------------------------------
# 4. range arguments at their edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_ranges_and_ranges_outside_the_slab(nvlib, scheme, dtype, tvopt):
    """chunk_count = 0 / z_count = 0: status 0, scalars exactly 0.0 (both words under TV_CP_FID_BOTH), every array untouched; a range
    outside the slab: TV_E_ARG, nothing written, tv_last_error() says why."""
    import torch
    nv, lib = nvlib, nvlib.lib()
    tvopt("TV_ZCHUNK", 2)
    shape = (7, 3, 10, 64)
    P = problem(scheme, shape, dtype)
    g = _geom(nv, P)
    nz, nch = shape[0], (shape[0] + 1) // 2
    for variant in ALL_VARIANTS:
        alg = Alg(nv, variant)
        words = 1 if alg.kind == "cpop" else (3 if (alg.kind == "cp" and alg.opt & FID_BOTH) else 2)
        for cb in (0, 1, nch):
            s, sc = alg.state(P), _scalars(1, 3, 123.0)
            before = {k: v.clone() for k, v in s.items()}
            assert alg.sweep(g, s, None, None, cb, 0, sc[0]) == 0, (variant, cb)
            assert all(torch.equal(s[k], before[k]) for k in s), (variant, cb)
            assert sc[0].tolist() == [0.0] * words + [123.0] * (3 - words), (variant, cb, sc)
        for cb, cc in ((-1, 1), (nch - 1, 2), (nch, 1), (0, nch + 1)):
            s, sc = alg.state(P), _scalars(1, 3, 123.0)
            before = {k: v.clone() for k, v in s.items()}
            assert alg.sweep(g, s, None, None, cb, cc, sc[0]) == E_ARG, (variant, cb, cc)
            assert len(lib.tv_last_error()) > 0
            assert all(torch.equal(s[k], before[k]) for k in s) and bool((sc == 123.0).all()), (variant, cb, cc)
        s = alg.state(P)
        nv.check(alg.sweep(g, s, None, None, 0, -1, _scalars(1, 3)[0]))
        before = {k: v.clone() for k, v in s.items()}
        for zb in (0, 3, nz):
            sc = _scalars(1, 1, 123.0)
            assert alg.fixup(g, s, None, None, zb, 0, sc[0]) == 0, (variant, zb)
            assert all(torch.equal(s[k], before[k]) for k in s), (variant, zb)
            assert sc.item() == (123.0 if alg.kind == "cpop" else 0.0), (variant, zb, sc)
        for zb, zn in ((nz - 1, 2), (nz, 1), (-1, 1), (0, nz + 1)):
            sc = _scalars(1, 1, 123.0)
            assert alg.fixup(g, s, None, None, zb, zn, sc[0]) == E_ARG, (variant, zb, zn)
            assert len(lib.tv_last_error()) > 0
            assert all(torch.equal(s[k], before[k]) for k in s) and sc.item() == 123.0, (variant, zb, zn)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_plane_slab_and_one_plane_volume(nvlib, scheme, dtype, tvopt):
    """nz = 1: one chunk, one plane, the whole range -- unsharded (no z axis) against the float64 reference, explicit range (0, 1) ==
    (0, -1); and as the middle slab of three planes with both halos (TV_ZCHUNK = 1: the unsharded chunks are the slabs, bit for bit)."""
    import torch
    nv = nvlib
    tvopt("TV_ZCHUNK", 1)
    P1 = problem(scheme, (1, 3, 10, 64), dtype)
    g1 = _geom(nv, P1)
    assert nv.lib().tv_cp_zchunk(g1.ref) == 1
    P3 = problem(scheme, (3, 3, 10, 64), dtype)
    g3 = _geom(nv, P3)
    for variant in ALL_VARIANTS:
        alg = Alg(nv, variant)
        s0, s1 = alg.state(P1), alg.state(P1)
        sw0, fx0 = run_ranges(nv, alg, g1, s0, [(0, -1)], [(0, -1)])
        alg.check_reference(P1, alg.out(s0), sw0, fx0, "nz = 1")
        sw1, fx1 = run_ranges(nv, alg, g1, s1, [(0, 1)], [(0, 1)])
        assert all(torch.equal(s1[k], s0[k]) for k in alg.outputs) and np.array_equal(sw1, sw0) and fx1 == fx0, variant
        s3 = alg.state(P3)
        sw3, fx3 = run_ranges(nv, alg, g3, s3, [(0, -1)], [(0, -1)])
        alg.check_reference(P3, alg.out(s3), sw3, fx3, "nz = 3")
        check_slabs(nv, alg, P3, (0, 1, 2, 3), 1, (alg.out(s3), sw3, fx3))
