"""Channel-coupled (vectorial) TV on the GPU (``-m gpu``): tv_cp_dual_vtv and tv_dual_gap_vtv through the C-ABI against the fp64 NumPy reference
of tests/test_cp_vtv_inputs.py (the joint projection with ``np.where`` and a division, the certificate site by site), the invariants of the
projection (inside the ball: the kernel's own v bit for bit; never beyond the radius), the register form against the generic form bit for bit, M = 1
against tv_cp_dual_wtv, the coupling itself (the result differs from the per-frame tv_cp_dual exactly where it must), z-ranges against the whole
volume, and ``VectorialTVChambollePock`` / ``denoise_tv_vectorial`` against the restated loop, with a known answer.

Tolerances are the project's (tests/test_gpu_cp_wtv.py): arrays to RTOL[dtype] * max|ref| with RTOL 1e-5 (fp32) / 1e-11 (fp64), scalars to
RTOL[dtype] * sum |terms|; trajectories: fp64 loss rtol 1e-10 and result 1e-9 * max|x0|, fp32 loss rtol 1e-5 and result rtol 1e-5 / atol 2e-3 on
fp32-rounded input; a feasible pair's gap >= -16 eps_dtype * primal; |q_s|_F <= lambda (1 + 8 eps_dtype) after the projection."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_cp_vtv_inputs import (LAM, SHAPES, SIGMA, WEIGHTINGS, Z_SHAPES, Z_WEIGHTINGS, kernel_inputs, np_vectorial, ref_dual, ref_gap,
                                ref_gap_parts, shares, site_norm)
from test_gpu_cp_wtv import (DTYPES, RTOL, WS_FILL, _bits, _explicit_pitch, _geometry, _pads_are_zero, _storage, _uploaders, _untouched,
                             _ws_beyond_the_partials_untouched, _z_channels, noisy_square)
from test_gpu_cp_wtv import gpu_dual as gpu_dual_per_frame      # tv_cp_dual_wtv (g an array) / tv_cp_dual (g None)

pytestmark = pytest.mark.gpu

PITCHED = ((3, 2, 16, 20), (2, 3, 9, 13))                       # the shapes that also run with an explicit pitch


def gpu_dual(x, q, sigma, lam, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None):
    """tv_cp_dual_vtv on local planes [a, b) (whole volume by default), halo planes of x passed by hand.  Returns (q after the call, the
    scalar).  keep / drop_halo as in tests/test_gpu_cp_wtv.py"""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    geo = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(geo)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]),
               xp=img(x[a - 1:a]) if (a > 0 and geo.z_active and drop_halo != "prev") else None,
               xn=img(x[b:b + 1]) if (b < nzg and geo.z_active and drop_halo != "next") else None)
    ws = geo.workspace()
    ws.fill_(WS_FILL)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None}, ws=ws)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_dual_vtv(geo.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), float(sigma), float(lam),
                                     out.data_ptr(), nv.ptr(ws), nv.current_stream(geo.device)))
    return dev["q"].cpu().numpy(), float(out.item())


def gpu_gap(x, q, x0, lam, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None):
    """tv_dual_gap_vtv on local planes [a, b), halo planes of x and q passed by hand; returns the three scalars"""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    geo = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(geo)
    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]), x0=img(x0[a:b]),
               xp=img(x[a - 1:a]) if (a > 0 and geo.z_active) else None, xn=img(x[b:b + 1]) if (b < nzg and geo.z_active) else None,
               qp=img(q[a - 1:a, cb]) if (a > 0 and geo.z_active) else None, qn=img(q[b:b + 1, cf]) if (b < nzg and geo.z_active) else None)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None})
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_dual_gap_vtv(geo.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), nv.ptr(dev["qp"]),
                                      nv.ptr(dev["qn"]), nv.ptr(dev["x0"]), float(lam), out.data_ptr(), nv.ptr(geo.workspace()),
                                      nv.current_stream(geo.device)))
    return tuple(out.cpu().tolist())


GAP_INPUTS = ("x", "q", "x0", "xp", "xn", "qp", "qn")


def _sites(mask, like):
    """a mask over the spatial sites (Nz, Ny, Nx) broadcast over the channels and frames of a gradient-like array"""
    return np.broadcast_to(mask[:, None, None], like.shape)


# ------------------------------------------------------------------------------------------------
# 1. tv_cp_dual_vtv: parity against the reference, and the projection invariants; both kernel forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_dual_entry_point_matches_the_reference(shape, scheme, dtype, tvopt):
    """every weighting, natural pitch (and an explicit one on two shapes), the default form and the generic form forced (TV_VTV_FORM = 2): q
    against the NumPy joint projection, the scalar against sum_s |D x_bar|_F, inside sites bit for bit against the v of tv_cp_dual_wtv (g = 1, a
    radius nothing reaches), |q_s|_F <= LAM (1 + 8 eps), inputs and pads untouched; the two forms give the same q and the same scalar bit for
    bit (where the default IS the generic form the two calls run the same kernel)"""
    rtol, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    ones = np.ones(shape, dtype=dtype)
    for weighting in WEIGHTINGS:
        x, q, _, kw = kernel_inputs(shape, scheme, dtype, weighting)
        wq, wvtv, v, n = ref_dual(x, q, SIGMA, LAM, scheme, kw)
        tol = rtol * float(np.max(np.abs(wq)))
        inside = _sites(n < LAM * (1.0 - 10.0 * rtol), v)
        assert float(np.mean(inside)) >= 0.02 and float(np.max(n)) < 1e6 * LAM
        for pitch in ((0, 0),) + ((_explicit_pitch(shape, dtype),) if shape in PITCHED else ()):
            gv, _ = gpu_dual_per_frame(x, q, ones, SIGMA, 1e6 * LAM, scheme, dtype, kw, pitch=pitch)      # the kernel's own v, nothing projected
            assert float(np.max(np.abs(gv - v))) <= rtol * float(np.max(np.abs(v)))
            got = {}
            for form in (0, 2):
                tvopt("TV_VTV_FORM", form)
                what = "%s %s pitch %r form %d" % (weighting, scheme, pitch, form)
                keep = {}
                gq, vtv = gpu_dual(x, q, SIGMA, LAM, scheme, dtype, kw, pitch=pitch, keep=keep)
                gn = site_norm(gq.astype(np.float64))
                print("%s: max|dq| %.3e (tol %.3e)  |d vtv| %.3e (tol %.3e)  max |q_s|_F / lam - 1 = %.3e (%.1f eps)" % (
                    what, np.max(np.abs(gq - wq)), tol, abs(vtv - wvtv), rtol * wvtv, np.max(gn) / LAM - 1.0, (np.max(gn) / LAM - 1.0) / eps))
                assert gq.dtype == dtype and np.isfinite(gq).all()
                assert float(np.max(np.abs(gq - wq))) <= tol, what
                assert abs(vtv - wvtv) <= rtol * wvtv, what                 # (every term of the sum is >= 0)
                assert float(np.max(gn)) <= LAM * (1.0 + 8.0 * eps), what
                np.testing.assert_array_equal(_bits(gq)[inside], _bits(gv)[inside], err_msg=what)
                _untouched(keep, ("x", "xp", "xn"))
                _ws_beyond_the_partials_untouched(keep["ws"])
                if pitch != (0, 0):
                    _pads_are_zero(keep["dev"]["q"])
                got[form] = (gq, vtv)
            np.testing.assert_array_equal(_bits(got[0][0]), _bits(got[2][0]), err_msg="%s %s pitch %r: register / generic form" % (weighting, scheme, pitch))
            assert got[0][1] == got[2][1]                                   # the same terms summed in the same order


# ------------------------------------------------------------------------------------------------
# 2. M = 1 is tv_cp_dual_wtv with g = 1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_frame_equals_the_adaptive_dual_step_with_unit_weights(scheme, dtype):
    shape, rtol = (1, 1, 32, 40), RTOL[dtype]
    x, q, _, kw = kernel_inputs(shape, scheme, dtype, "plain")
    n = ref_dual(x, q, SIGMA, LAM, scheme, kw)[3]
    got = gpu_dual(x, q, SIGMA, LAM, scheme, dtype, kw)
    wtv = gpu_dual_per_frame(x, q, np.ones(shape, dtype=dtype), SIGMA, LAM, scheme, dtype, kw)
    print("%s %s: max|dq| %.3e  scalars %.12e %.12e" % (scheme, np.dtype(dtype).name, np.max(np.abs(got[0] - wtv[0])), got[1], wtv[1]))
    assert float(np.max(np.abs(got[0] - wtv[0]))) <= rtol * float(np.max(np.abs(wtv[0])))
    assert abs(got[1] - wtv[1]) <= rtol * wtv[1]
    inside = _sites(n < LAM * (1.0 - 10.0 * rtol), got[0])
    np.testing.assert_array_equal(_bits(got[0])[inside], _bits(wtv[0])[inside])


# ------------------------------------------------------------------------------------------------
# 3. the coupling: not the per-frame projection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] >= 2])
def test_result_differs_from_the_per_frame_projection_where_it_must(shape, scheme, dtype):
    """at every site whose joint norm exceeds LAM (by 0.1 %) while one of its frames lies inside its own ball (by 0.1 %), that frame of
    tv_cp_dual's result is v itself and the joint result is v times a factor < 1: the two differ at every such site"""
    x, q, _, kw = kernel_inputs(shape, scheme, dtype, "plain")
    v = ref_dual(x, q, SIGMA, LAM, scheme, kw)[2]
    n, nf = site_norm(v), np.sqrt(np.sum(v * v, axis=1))
    coupled = (n > LAM * 1.001) & np.any((nf < LAM * 0.999) & (nf > 0.0), axis=1)
    assert float(np.mean(coupled)) >= 0.02
    joint, _ = gpu_dual(x, q, SIGMA, LAM, scheme, dtype, kw)
    per_frame, _ = gpu_dual_per_frame(x, q, None, SIGMA, LAM, scheme, dtype, kw)
    differs = np.any(joint != per_frame, axis=(1, 2))
    print("%s %s %s: coupled sites %.3f, differing sites %.3f" % (shape, scheme, np.dtype(dtype).name, np.mean(coupled), np.mean(differs)))
    assert bool(np.all(differs[coupled]))
    assert float(np.max(site_norm(per_frame.astype(np.float64)))) > LAM * 1.001         # ... and the per-frame result is not jointly feasible


# ------------------------------------------------------------------------------------------------
# 4. z-ranges: planes [a, b) with hand-passed halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
# Z_SHAPES (tests/test_cp_vtv_inputs.py, where every plane of them is shown to hold all three classes of sites): register form, generic form
Z_RANGES = ((0, 2), (2, 5), (1, 4), (0, 1), (2, 3), (4, 5))    # (2, 3): one plane with both halo planes at once, what a one-plane rank gets
Z_CUTS = ((0, 2, 5), (0, 1, 4, 5), (0, 1, 2, 3, 4, 5))         # partitions of [0, 5) into z-ranges; the last: every range is one plane


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", Z_SHAPES)
def test_dual_z_ranges_equal_the_whole_volume(shape, scheme, dtype, tvopt):
    """every weighting of ``Z_WEIGHTINGS`` (the per-voxel time weight is cut by planes with the range), the default form and the generic form
    forced: q of a range is bit for bit the planes of the whole-volume call, inputs and halo planes are untouched, and the scalars of the
    ranges of a partition of [0, 5) -- (0, 2) + (2, 5), (0, 1) + (1, 4) + (4, 5) -- add up to the whole's"""
    for weighting in Z_WEIGHTINGS:
        x, q, _, kw = kernel_inputs(shape, scheme, dtype, weighting)
        for form in (0, 2):
            tvopt("TV_VTV_FORM", form)
            what = "%s %s %s form %d" % (weighting, scheme, np.dtype(dtype).name, form)
            wq, wvtv = gpu_dual(x, q, SIGMA, LAM, scheme, dtype, kw)
            parts = {}
            for a, b in Z_RANGES:
                keep = {}
                gq, vtv = gpu_dual(x, q, SIGMA, LAM, scheme, dtype, kw, z_range=(a, b), keep=keep)
                np.testing.assert_array_equal(_bits(gq), _bits(wq[a:b]), err_msg="%s planes [%d, %d)" % (what, a, b))
                _untouched(keep, ("x", "xp", "xn"))
                parts[(a, b)] = vtv
            print("%s: parts %.17g + %.17g whole %.17g" % (what, parts[(0, 2)], parts[(2, 5)], wvtv))
            assert abs(parts[(0, 2)] + parts[(2, 5)] - wvtv) <= 1e-12 * wvtv, what
            assert abs(parts[(0, 1)] + parts[(1, 4)] + parts[(4, 5)] - wvtv) <= 1e-12 * wvtv, what


@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    """both forms (``Z_SHAPES``), a range of three planes and a range of one"""
    # a forward difference reads the next slab, a backward one the previous (central, hybrid: both)
    sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))
    for shape in Z_SHAPES:
        x, q, _, kw = kernel_inputs(shape, scheme, np.float32, "plain")
        for z_range in ((1, 4), (2, 3)):
            for side in sides:
                keep = {}
                with pytest.raises(ValueError, match=r"x_%s.*halo.*code -2" % side):
                    gpu_dual(x, q, SIGMA, LAM, scheme, np.float32, kw, z_range=z_range, keep=keep, drop_halo=side)
                torch.cuda.synchronize()
                _untouched(keep, ("x", "q", "xp", "xn"))
                assert bool((keep["ws"] == WS_FILL).all())


# ------------------------------------------------------------------------------------------------
# 5. tv_dual_gap_vtv
# ------------------------------------------------------------------------------------------------
def _check_gap(got, ref, dtype, what):
    rtol, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    vtv, fid, gap, terms = ref
    print("%s got %r ref %r  |d gap| %.3e (tol %.3e)" % (what, tuple(got), ref[:3], abs(got[2] - gap), rtol * terms))
    assert abs(got[0] - vtv) <= rtol * vtv, what
    assert abs(got[1] - fid) <= rtol * fid, what
    assert abs(got[2] - gap) <= rtol * terms, what
    assert got[2] >= -16.0 * eps * (fid + LAM * vtv), what              # a feasible q: the gap is >= 0 up to the fp floor


@functools.lru_cache(maxsize=None)
def feasible_q(shape, scheme, dtype, weighting):
    """the output of the dual step's reference, shrunk by 4 eps and rounded to the dtype: |q_s|_F <= LAM per spatial site"""
    x, q, _, kw = kernel_inputs(shape, scheme, dtype, weighting)
    fq = (ref_dual(x, q, SIGMA, LAM, scheme, kw)[0] * (1.0 - 4.0 * float(np.finfo(dtype).eps))).astype(dtype)
    assert float(np.max(site_norm(fq.astype(np.float64)))) <= LAM
    fq.setflags(write=False)
    return fq


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gap_matches_the_reference_and_writes_nothing(shape, scheme, dtype):
    for weighting in WEIGHTINGS:
        x, _, x0, kw = kernel_inputs(shape, scheme, dtype, weighting)
        q = feasible_q(shape, scheme, dtype, weighting)
        _, sq, reg_part, _ = ref_gap_parts(x, q, x0, LAM, scheme, kw)
        assert float(np.min(sq)) >= 0.0 and float(np.min(reg_part)) >= -1e-12 * LAM      # both parts >= 0 site by site on a feasible q
        ref = ref_gap(x, q, x0, LAM, scheme, kw)
        for pitch in ((0, 0),) + ((_explicit_pitch(shape, dtype),) if shape in PITCHED else ()):
            keep = {}
            got = gpu_gap(x, q, x0, LAM, scheme, dtype, kw, pitch=pitch, keep=keep)
            _check_gap(got, ref, dtype, "%s %s pitch %r" % (weighting, scheme, pitch))
            _untouched(keep, GAP_INPUTS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_gap_z_range_partials_add_up(scheme, dtype):
    """M = 2 and the generic count M = 9 (the frame loop over q_prev / q_next), plain and under a per-voxel time weight cut by planes with
    the range; ``Z_CUTS``: the last cut hands every call one plane, the inner ones with both halo planes of x and of q at once"""
    for shape in Z_SHAPES:
        for weighting in ("plain", "weight_vol"):
            x, _, x0, kw = kernel_inputs(shape, scheme, dtype, weighting)
            q = feasible_q(shape, scheme, dtype, weighting)
            ref = ref_gap(x, q, x0, LAM, scheme, kw)
            whole = gpu_gap(x, q, x0, LAM, scheme, dtype, kw)
            _check_gap(whole, ref, dtype, "%s %s whole" % (shape, weighting))
            for cut in Z_CUTS:
                parts = np.zeros(3)
                for a, b in zip(cut[:-1], cut[1:]):
                    keep = {}
                    parts += np.array(gpu_gap(x, q, x0, LAM, scheme, dtype, kw, z_range=(a, b), keep=keep))
                    _untouched(keep, GAP_INPUTS)
                print("%s %s %s %s cut %r: parts %r whole %r" % (shape, weighting, scheme, np.dtype(dtype).name, cut, tuple(parts), whole))
                for k, scale in enumerate((ref[0], ref[1], ref[3])):
                    assert abs(parts[k] - whole[k]) <= 1e-12 * scale, (shape, weighting, cut, k)


# ------------------------------------------------------------------------------------------------
# 6. solver
# ------------------------------------------------------------------------------------------------
REG = 10.0
TRAJ_SHAPES = [(3, 2, 16, 20), (2, 9, 9, 13)]                  # register form on lanes; generic form on scalar rows


def _kw_of(shape):
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


@functools.lru_cache(maxsize=None)
def coupled_square(shape):
    """the centred square of tests/test_gpu_cp_huber.py's noisy_square with a contrast that falls from frame to frame (100, 50, 33, ...) under
    the same N(0, 10^2) noise: strong and weak channels of one object"""
    ny, nx = shape[2:]
    clean = np.zeros(shape)
    clean[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    out = clean / (1.0 + np.arange(shape[1]))[None, :, None, None] + (noisy_square(shape) - clean)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, n_iter, f32_input=False):
    x0 = coupled_square(shape)
    if f32_input:
        x0 = x0.astype(np.float32).astype(np.float64)
    return np_vectorial(x0, n_iter, REG, scheme, _kw_of(shape))


def _solver(pytv, shape, dtype, scheme, reg=REG, **how):
    return pytv.solvers.VectorialTVChambollePock(torch.as_tensor(coupled_square(shape).astype(dtype)).cuda(), reg, scheme=scheme,
                                                 **_kw_of(shape), **how)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme):
    import pytv
    wx, wloss, state = np_trajectory(shape, scheme, 20)
    cp = _solver(pytv, shape, np.float64, scheme)
    assert cp.it == 0 and cp.gamma == 1.0 and cp.fused is False and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape))
    with pytest.raises(ValueError, match="VectorialTVChambollePock.*one-sweep"):
        cp.set_fused(True)
    loss = cp.run(20)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(coupled_square(shape))))
    assert cp.it == 20 and cp.fused is False
    # duality_gap() against the certificate of the restated pair
    wvtv, wfid, wgap, wterms = ref_gap(state[0], state[2], coupled_square(shape), REG, scheme, _kw_of(shape))
    primal, dual, gap = cp.duality_gap()
    print("   primal %.12e (ref %.12e)  gap %.6e (ref %.6e)" % (primal, wfid + REG * wvtv, gap, wgap))
    np.testing.assert_allclose(primal, wfid + REG * wvtv, rtol=1e-10)
    assert abs(gap - wgap) <= 1e-9 * wterms and gap > 0.0 and dual == primal - gap
    # reset() restarts the schedule: the first run again, bit for bit
    q_end, x_end = cp.q.clone(), cp.result().clone()
    cp.reset()
    assert cp.it == 0 and torch.equal(cp.x, cp.x0) and torch.equal(cp.x_bar, cp.x0) and not bool(cp.q.any())
    np.testing.assert_array_equal(cp.run(20), loss)
    assert torch.equal(cp.result(), x_end) and torch.equal(cp.q, q_end)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_solver_trajectory_fp32(scheme):
    """the fp32 tolerance of tests/test_gpu_cp_wtv.py against the fp64 restatement on the fp32-rounded input"""
    import pytv
    shape = TRAJ_SHAPES[0]
    wx, wloss, _ = np_trajectory(shape, scheme, 20, f32_input=True)
    cp = _solver(pytv, shape, np.float32, scheme)
    loss = cp.run(20)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
def test_run_until_converges_in_fp64(scheme):
    import pytv
    cp = _solver(pytv, (3, 2, 16, 20), np.float64, scheme)
    loss, info = cp.run_until(1e-6, 2000, 50)
    print(scheme, info)
    assert info["converged"] is True and len(loss) == info["iterations"] == cp.it and info["iterations"] % 50 == 0
    assert 0.0 <= info["gap"] <= 1e-6 * info["primal"] and info["dual"] == info["primal"] - info["gap"]
    assert info["error_bound"] == np.sqrt(2 * info["gap"])
    state = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
    assert cp.duality_gap() == (info["primal"], info["dual"], info["gap"])          # the certificate leaves the state of the loop alone
    assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q)))


def test_constructor_refuses_bad_regularization():
    import pytv
    x0 = torch.as_tensor(np.array(noisy_square((1, 2, 8, 12)))).cuda()
    for reg in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="regularization"):
            pytv.solvers.VectorialTVChambollePock(x0, reg)


# ------------------------------------------------------------------------------------------------
# 7. known answer: M identical frames are single-frame TV at weight / sqrt(M)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_four_identical_frames_are_single_frame_tv_at_half_the_weight(scheme, dtype):
    """|.|_F = sqrt(M) |.|_2 on identical frames, so with reg_time = 0 the iterates of the joint solver at weight REG coincide, in exact
    arithmetic, with ``AcceleratedChambollePock`` on one frame at REG / 2 (same L^2: the time channel is off, same schedule).  To the solver
    tolerance after 30 iterations; the weight-REG single-frame run is far away"""
    import pytv
    frame = np.array(noisy_square((3, 1, 16, 20))).astype(dtype)
    x0 = np.repeat(frame, 4, axis=1)
    kw = dict(reg_z_over_reg=0.7, reg_time=0.0)
    joint = pytv.solvers.VectorialTVChambollePock(torch.as_tensor(x0).cuda(), REG, scheme=scheme, **kw)
    runs = {}
    for w in (REG / 2.0, REG):
        acc = pytv.solvers.AcceleratedChambollePock(torch.as_tensor(frame).cuda(), w, scheme=scheme, **kw)
        acc.set_fused(False)
        acc.run(30)
        runs[w] = acc.result().cpu().numpy().astype(np.float64)[:, 0]
    assert joint.L2 == acc.L2
    joint.run(30)
    got = joint.result().cpu().numpy().astype(np.float64)
    err = max(float(np.max(np.abs(got[:, m] - runs[REG / 2.0]))) for m in range(4))
    far = float(np.max(np.abs(got[:, 0] - runs[REG])))
    print("%s %s: max|x_m - single(REG / 2)| %.3e, max|x_0 - single(REG)| %.3e" % (scheme, np.dtype(dtype).name, err, far))
    if dtype == np.float64:
        assert err <= 1e-9 * float(np.max(np.abs(frame)))
    else:
        for m in range(4):
            np.testing.assert_allclose(got[:, m], runs[REG / 2.0], rtol=1e-5, atol=2e-3)
    assert far > 0.1                                                    # a kernel that forgets the coupling lands here instead


# ------------------------------------------------------------------------------------------------
# 8. front-end
# ------------------------------------------------------------------------------------------------
def test_denoise_tv_vectorial_front_end():
    import pytv
    rng = np.random.default_rng(2)
    chw = (np.array(coupled_square((1, 3, 24, 28)))[0] + rng.standard_normal((3, 24, 28))).astype(np.float32)
    out = pytv.denoise_tv_vectorial(chw, 10.0, rel_gap=1e-3, max_num_iter=400)
    ref = pytv.solvers.VectorialTVChambollePock(torch.as_tensor(chw[None]).cuda(), 10.0, scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-3, 400, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] < 400
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == chw.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy()[0])
    assert float(np.max(np.abs(out - chw))) > 1.0                       # it denoised
    # channel_axis = -1: (H, W, C) in, (H, W, C) out, the same image
    hwc = np.ascontiguousarray(np.moveaxis(chw, 0, -1))
    last = pytv.denoise_tv_vectorial(hwc, 10.0, channel_axis=-1, rel_gap=1e-3, max_num_iter=400)
    assert last.shape == hwc.shape and last.dtype == np.float32
    np.testing.assert_array_equal(np.moveaxis(last, -1, 0), out)
    # 4-D: (Nz, C, H, W) with channel_axis = 1, fp64, never converges: exactly 40 iterations, the solver's run(40)
    vol = np.array(coupled_square((3, 2, 16, 20)))
    out4 = pytv.denoise_tv_vectorial(vol, 10.0, channel_axis=1, rel_gap=-1.0, max_num_iter=40, scheme="hybrid", check_every=20)
    ref = pytv.solvers.VectorialTVChambollePock(torch.as_tensor(vol.copy()).cuda(), 10.0, scheme="hybrid", reg_z_over_reg=1.0)
    ref.run(40)
    assert out4.shape == vol.shape and out4.dtype == np.float64
    np.testing.assert_array_equal(out4, ref.result().cpu().numpy())
    # torch in -> device tensor out; other ranks refused
    t = pytv.denoise_tv_vectorial(torch.as_tensor(chw).cuda(), 10.0, rel_gap=1e-3, max_num_iter=400)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == chw.shape and np.array_equal(t.cpu().numpy(), out)
    for bad in (np.zeros((8, 8), dtype=np.float32), np.zeros((1, 1, 2, 8, 8), dtype=np.float32)):
        with pytest.raises(ValueError, match="3-D"):
            pytv.denoise_tv_vectorial(bad)
