"""The Huber-TV regulariser on the GPU (``-m gpu``): tv_cp_dual_huber and tv_dual_gap_huber through the C-ABI against fp64 NumPy restatements
built on ``orc.D`` / ``orc.D_T`` (textbook formulas: a division where the kernel multiplies by a host-formed constant, ``np.where`` where it
clamps, the gap never as a perfect square), the projection invariants, z-ranges against the whole volume, the plane-marching form against
the one-site form, and ``HuberChambollePock`` / ``denoise_tv_huber`` against a NumPy restatement of Algorithm 3 of Chambolle & Pock 2011 --
trajectory, certified stop, the rate against the accelerated plain-TV solver, and that the model does what it is for: fewer flat steps on a ramp.

Tolerances are the project's (tests/test_gpu_cp_prox.py, tests/test_gpu_cp_accel.py): arrays to RTOL[dtype] * max|ref| with RTOL 1e-5 (fp32) /
1e-11 (fp64), scalars to RTOL[dtype] * sum |terms| of the sum they are; trajectories: fp64 loss rtol 1e-10 and result 1e-9 * max|x0|, fp32 loss
rtol 1e-5 and result rtol 1e-5 / atol 2e-3 on fp32-rounded input; a feasible pair's gap >= -16 eps_dtype * primal (the floor tests/
test_gpu_dual_gap.py uses for the cancellation the solvers' ``_GAP_DOC`` describes)."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_prox import (PARITY_SHAPES, WEIGHTINGS, _case_kw, _explicit_pitch, _pads_are_zero, _storage, _untouched, _z_channels,
                              make_inputs, np_project)

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
DTYPES = [np.float64, np.float32]
PLAIN_KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
LAM = 5.0                      # the radius of make_inputs' q
X_SCALE, SIGMA = 0.1, 16.0     # x of make_inputs (0..60) scaled to 0..6; a large dual step (Algorithm 3's sigma grows as alpha shrinks): |v| >
                               # lam at roughly the sites with |D x| > alpha, and the smallest of the four regime shares is 0.34 (sigma = 4: 0.10)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


# ------------------------------------------------------------------------------------------------
# the two kernels, restated in fp64
# ------------------------------------------------------------------------------------------------
def huber(n, alpha):
    return np.where(n <= alpha, n * n / (2.0 * alpha), n - 0.5 * alpha)


def ref_dual(x, q, sigma, lam, alpha, scheme, kw):
    """(q_new, sum h_alpha(|D x|), v, |D x|) in fp64: v the shrunk vector before the projection"""
    Dx = orc.D(np.asarray(x, dtype=np.float64), scheme, **kw)
    v = (np.asarray(q, dtype=np.float64) + sigma * Dx) / (1.0 + sigma * alpha / lam)
    n = np.sqrt(np.sum(Dx * Dx, axis=1))
    return np_project(v, lam), float(np.sum(huber(n, alpha))), v, n


def ref_gap(x, q, x0, lam, alpha, scheme, kw):
    """(sum h_alpha(|D x|), 1/2 |x - x0|^2, gap, sum |terms of the gap|) in fp64, the gap site by site as
    1/2 (x - x0 + D^T q)^2 + lam h_alpha(|D x|) - <q, D x> + (alpha / 2 lam) |q|^2"""
    x, q, x0 = (np.asarray(a, dtype=np.float64) for a in (x, q, x0))
    Dx = orc.D(x, scheme, **kw)
    r = x - x0 + orc.D_T(q, scheme, **kw)
    h = huber(np.sqrt(np.sum(Dx * Dx, axis=1)), alpha)
    dot, qq = np.sum(q * Dx, axis=1), np.sum(q * q, axis=1)
    gap = np.sum(0.5 * r * r) + np.sum(lam * h - dot + (0.5 * alpha / lam) * qq)
    terms = np.sum(0.5 * r * r) + np.sum(lam * h + np.abs(dot) + (0.5 * alpha / lam) * qq)
    return float(np.sum(h)), float(0.5 * np.sum((x - x0) ** 2)), float(gap), float(terms)


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, scheme, dtype, weighting):
    """x (scaled), a feasible q (|q|_2 <= LAM per site: projected random vectors) and x0 of tests/test_gpu_cp_prox.py's make_inputs, and alpha =
    the median of |D x|_2 over the sites, rounded to three decimals: half of the sites on either side of the Huber threshold"""
    kw = _case_kw(weighting, shape)
    x, q, x0, _ = make_inputs(shape, scheme, dtype, kw)
    x = (X_SCALE * x.astype(np.float64)).astype(dtype)
    x0 = (X_SCALE * x0.astype(np.float64)).astype(dtype)
    Dx = orc.D(x.astype(np.float64), scheme, **kw)
    alpha = round(float(np.median(np.sqrt(np.sum(Dx * Dx, axis=1)))), 3)
    for a in (x, q, x0):
        a.setflags(write=False)
    return x, q, x0, alpha, kw


def _geometry(nv, x, scheme, dtype, kw, pitch, a, b):
    nzg = x.shape[0]
    return nv.Geometry((b - a,) + tuple(x.shape[1:]), scheme, _tdt(dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1],
                       **({k: (v[a:b] if (isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg and v.dtype != bool) else v)
                           for k, v in kw.items()}))


def _uploaders(g):
    def img(arr):
        t = g.new_image(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    def grad(arr):
        t = g.new_grad(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t
    return img, grad


WS_FILL = -7.0


def gpu_dual(x, q, sigma, lam, alpha, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None):
    """tv_cp_dual_huber on local planes [a, b) (whole volume by default), halo planes of x passed by hand.  Returns (q after the call, the
    scalar).  keep: receives the device tensors, copies of their storage made before the call, and the workspace (filled with WS_FILL before
    the call).  drop_halo: "prev" / "next" -- pass NULL for that halo plane."""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(g)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]),
               xp=img(x[a - 1:a]) if (a > 0 and g.z_active and drop_halo != "prev") else None,
               xn=img(x[b:b + 1]) if (b < nzg and g.z_active and drop_halo != "next") else None)
    ws = g.workspace()
    ws.fill_(WS_FILL)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None}, ws=ws)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_dual_huber(g.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), float(sigma), float(lam),
                                       float(alpha), out.data_ptr(), nv.ptr(ws), nv.current_stream(g.device)))
    return dev["q"].cpu().numpy(), float(out.item())


def gpu_gap(x, q, x0, lam, alpha, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None):
    """tv_dual_gap_huber on local planes [a, b), halo planes of x and q passed by hand; returns the three scalars"""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = _geometry(nv, x, scheme, dtype, kw, pitch, a, b)
    img, grad = _uploaders(g)
    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]), x0=img(x0[a:b]),
               xp=img(x[a - 1:a]) if (a > 0 and g.z_active) else None, xn=img(x[b:b + 1]) if (b < nzg and g.z_active) else None,
               qp=img(q[a - 1:a, cb]) if (a > 0 and g.z_active) else None, qn=img(q[b:b + 1, cf]) if (b < nzg and g.z_active) else None)
    if keep is not None:
        keep.update(dev=dev, before={k: _storage(v).clone() for k, v in dev.items() if v is not None})
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_dual_gap_huber(g.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), nv.ptr(dev["qp"]),
                                        nv.ptr(dev["qn"]), nv.ptr(dev["x0"]), float(lam), float(alpha), out.data_ptr(), nv.ptr(g.workspace()),
                                        nv.current_stream(g.device)))
    return tuple(out.cpu().tolist())


def _ws_beyond_the_partials_untouched(ws):
    """the call reduces through slot 0 of the three equal slots of the workspace (csrc/tv_host.h, Partials): the other two keep the fill"""
    n = ws.numel() // 3
    assert bool((ws[n + 16:] == WS_FILL).all())


GAP_INPUTS = ("x", "q", "x0", "xp", "xn", "qp", "qn")


# ------------------------------------------------------------------------------------------------
# 1. tv_cp_dual_huber: parity against the restatement, and the projection invariants
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_dual_entry_point_matches_the_restatement(shape, scheme, dtype):
    """every weighting, natural and explicit pitch.  Invariants of the projection: |q|_2 <= lam (1 + RTOL) at every site afterwards, and where the
    restatement has |v| < lam (1 - 10 RTOL) the new q is v itself within the array tolerance -- no spurious projection"""
    rtol = RTOL[dtype]
    for weighting in WEIGHTINGS:
        x, q, _, alpha, kw = kernel_inputs(shape, scheme, dtype, weighting)
        wq, whub, v, n = ref_dual(x, q, SIGMA, LAM, alpha, scheme, kw)
        nv_ = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
        shares = (np.mean(n <= alpha), np.mean(n > alpha), np.mean(nv_ <= LAM), np.mean(nv_ > LAM))
        assert min(shares) >= 0.1, shares                               # |D x| below / above alpha, |v| below / above lam
        tol = rtol * float(np.max(np.abs(wq)))
        inside = np.broadcast_to(nv_ < LAM * (1.0 - 10.0 * rtol), v.shape)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            what = "%s %s pitch %r" % (weighting, scheme, pitch)
            keep = {}
            gq, hub = gpu_dual(x, q, SIGMA, LAM, alpha, scheme, dtype, kw, pitch=pitch, keep=keep)
            gn = np.sqrt(np.sum(gq.astype(np.float64) ** 2, axis=1))
            print("%s: alpha %.3f  max|dq| %.3e (tol %.3e)  |d hub| %.3e (tol %.3e)  max|q|/lam - 1 %.3e  regimes %.2f %.2f %.2f %.2f" % (
                what, alpha, np.max(np.abs(gq - wq)), tol, abs(hub - whub), rtol * whub, np.max(gn) / LAM - 1.0, *shares))
            assert gq.dtype == dtype
            assert float(np.max(np.abs(gq - wq))) <= tol, what
            assert abs(hub - whub) <= rtol * whub, what                 # (every term of the sum is >= 0)
            assert float(np.max(gn)) <= LAM * (1.0 + rtol), what
            assert float(np.max(np.abs(gq - v)[inside])) <= tol, what
            _untouched(keep, ("x", "xp", "xn"))
            _ws_beyond_the_partials_untouched(keep["ws"])
            if pitch != (0, 0):
                _pads_are_zero(keep["dev"]["q"])


# ------------------------------------------------------------------------------------------------
# 2. z-ranges: planes [a, b) with hand-passed halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
Z_SHAPE = (5, 2, 16, 20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_z_ranges_equal_the_whole_volume(scheme, dtype):
    x, q, _, alpha, kw = kernel_inputs(Z_SHAPE, scheme, dtype, "plain")
    wq, whub = gpu_dual(x, q, SIGMA, LAM, alpha, scheme, dtype, kw)
    n = ref_dual(x, q, SIGMA, LAM, alpha, scheme, kw)[3]
    parts = {}
    for a, b in ((0, 2), (2, 5), (1, 4)):
        keep = {}
        gq, hub = gpu_dual(x, q, SIGMA, LAM, alpha, scheme, dtype, kw, z_range=(a, b), keep=keep)
        np.testing.assert_array_equal(gq, wq[a:b], err_msg="planes [%d, %d)" % (a, b))
        _untouched(keep, ("x", "xp", "xn"))
        want = float(np.sum(huber(n[a:b], alpha)))                      # the restatement's share of those planes
        assert abs(hub - want) <= RTOL[dtype] * want, (a, b)
        parts[(a, b)] = hub
    print("%s %s: parts %.17g + %.17g whole %.17g" % (scheme, np.dtype(dtype).name, parts[(0, 2)], parts[(2, 5)], whub))
    assert abs(parts[(0, 2)] + parts[(2, 5)] - whub) <= RTOL[dtype] * whub


@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    x, q, _, alpha, kw = kernel_inputs(Z_SHAPE, scheme, np.float32, "plain")
    # a forward difference reads the next slab, a backward one the previous (central, hybrid: both)
    sides = {"upwind": ("next",), "downwind": ("prev",)}.get(scheme, ("prev", "next"))
    for side in sides:
        keep = {}
        with pytest.raises(ValueError, match=r"halo.*code -2"):
            gpu_dual(x, q, SIGMA, LAM, alpha, scheme, np.float32, kw, z_range=(1, 4), keep=keep, drop_halo=side)
        torch.cuda.synchronize()
        _untouched(keep, ("x", "q", "xp", "xn"))
        assert bool((keep["ws"] == WS_FILL).all())


# ------------------------------------------------------------------------------------------------
# 3. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dual_marching_form_equals_one_site_form(scheme, tvopt):
    """the equality tests/test_gpu_cp_accel.py's test_marching_form_equals_one_site_form asserts: arrays to 1e-5 max|.|, the scalar to 1e-5"""
    shape, dtype, alpha = (2, 2, 1024, 1024), np.float32, 2.0
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, shape[0], shape[1], **PLAIN_KW)
    x = 6.0 * rng.random(shape, dtype=np.float32)
    q = LAM * (rng.random((shape[0], nd) + shape[1:], dtype=np.float32) - 0.5)
    march = gpu_dual(x, q, SIGMA, LAM, alpha, scheme, dtype, PLAIN_KW)
    tvopt("TV_NO_MARCH", 1)
    site = gpu_dual(x, q, SIGMA, LAM, alpha, scheme, dtype, PLAIN_KW)
    tol = 1e-5 * float(np.max(np.abs(site[0])))
    moved = float(np.mean(site[0] != q))
    print("%s: max|dq| %.3e (tol %.3e)  hub %.9e / %.9e  entries changed %.3f" % (scheme, np.max(np.abs(march[0] - site[0])), tol, march[1], site[1],
                                                                              moved))
    assert float(np.max(np.abs(march[0] - site[0]))) <= tol
    assert abs(march[1] - site[1]) <= 1e-5 * site[1]
    assert np.isfinite(march[1]) and march[1] > 0.0 and moved > 0.9


# ------------------------------------------------------------------------------------------------
# 4. tv_dual_gap_huber
# ------------------------------------------------------------------------------------------------
def _check_gap(got, ref, dtype, what):
    rtol, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    hub, fid, gap, terms = ref
    print("%s got %r ref %r  |d gap| %.3e (tol %.3e)" % (what, tuple(got), ref[:3], abs(got[2] - gap), rtol * terms))
    assert abs(got[0] - hub) <= rtol * hub, what
    assert abs(got[1] - fid) <= rtol * fid, what
    assert abs(got[2] - gap) <= rtol * terms, what
    assert got[2] >= -16.0 * eps * (fid + LAM * hub), what              # a feasible q: the gap is >= 0 up to the fp floor


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_gap_matches_the_restatement_and_writes_nothing(shape, scheme, dtype):
    for weighting in WEIGHTINGS:
        x, q, x0, alpha, kw = kernel_inputs(shape, scheme, dtype, weighting)
        assert float(np.max(np.sum(q.astype(np.float64) ** 2, axis=1))) <= (LAM * (1.0 + 1e-6)) ** 2          # feasible by construction
        ref = ref_gap(x, q, x0, LAM, alpha, scheme, kw)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            keep = {}
            got = gpu_gap(x, q, x0, LAM, alpha, scheme, dtype, kw, pitch=pitch, keep=keep)
            _check_gap(got, ref, dtype, "%s %s pitch %r alpha %.3f" % (weighting, scheme, pitch, alpha))
            _untouched(keep, GAP_INPUTS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_gap_z_range_partials_add_up(scheme, dtype):
    x, q, x0, alpha, kw = kernel_inputs(Z_SHAPE, scheme, dtype, "plain")
    ref = ref_gap(x, q, x0, LAM, alpha, scheme, kw)
    whole = gpu_gap(x, q, x0, LAM, alpha, scheme, dtype, kw)
    _check_gap(whole, ref, dtype, "whole")
    for cut in ((0, 2, 5), (0, 1, 4, 5)):
        parts = np.zeros(3)
        for a, b in zip(cut[:-1], cut[1:]):
            keep = {}
            parts += np.array(gpu_gap(x, q, x0, LAM, alpha, scheme, dtype, kw, z_range=(a, b), keep=keep))
            _untouched(keep, GAP_INPUTS)
        print("%s %s cut %r: parts %r whole %r" % (scheme, np.dtype(dtype).name, cut, tuple(parts), whole))
        for k, scale in enumerate((ref[0], ref[1], ref[3])):
            assert abs(parts[k] - whole[k]) <= RTOL[dtype] * scale, (cut, k)


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 3) and of its duality gap
# ------------------------------------------------------------------------------------------------
REG = 10.0
ALPHAS = (0.5, 2.0)


def np_linear_steps(L2, gamma, delta):
    mu = 2.0 * np.sqrt(gamma * delta) / np.sqrt(L2)
    return mu / (2.0 * gamma), mu / (2.0 * delta), 1.0 / (1.0 + mu)


def np_huber_cp(x0, n_iter, lam, alpha, scheme, kw, gamma=1.0, state=None):
    """n_iter iterations from ``state`` = (x, x_bar, q) (default: the start); returns (x, loss, (x, x_bar, q))"""
    x0 = np.asarray(x0, dtype=np.float64)
    tau, sigma, theta = np_linear_steps(orc.normal_spectral_bound(scheme, x0.shape, **kw), gamma, alpha / lam)
    x, xb, q = (x0.copy(), x0.copy(), np.zeros_like(orc.D(x0, scheme, **kw))) if state is None else state
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project((q + sigma * Dxb) / (1.0 + sigma * alpha / lam), lam)
        xn = (x - tau * orc.D_T(q, scheme, **kw) + tau * x0) / (1.0 + tau)
        xb = xn + theta * (xn - x)
        x = xn
        loss[k] = 0.5 * np.sum((x - x0) ** 2) + lam * np.sum(huber(np.sqrt(np.sum(Dxb * Dxb, axis=1)), alpha))
    return x, loss, (x, xb, q)


def np_huber_gap(x, q, x0, lam, alpha, scheme, kw):
    """(primal, gap) in fp64"""
    hub, fid, gap, _ = ref_gap(x, q, x0, lam, alpha, scheme, kw)
    return fid + lam * hub, gap


def np_run_until(x0, rel_gap, max_iter, check_every, lam, alpha, scheme, kw):
    """the iteration count of ``run_until`` in the restatement, and its last (primal, gap)"""
    state, done = None, 0
    while True:
        _, _, state = np_huber_cp(x0, check_every, lam, alpha, scheme, kw, state=state)
        done += check_every
        primal, gap = np_huber_gap(state[0], state[2], x0, lam, alpha, scheme, kw)
        if gap <= rel_gap * primal or done >= max_iter:
            return done, primal, gap


@functools.lru_cache(maxsize=None)
def noisy_square(shape):
    """a centred square of height 100 plus N(0, 10^2) noise"""
    x = np.zeros(shape)
    ny, nx = shape[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    x = x + 10.0 * np.random.default_rng(0).standard_normal(shape)
    x.setflags(write=False)
    return x


def _kw_of(shape):
    return dict(reg_z_over_reg=0.7, reg_time=0.25) if shape[0] > 1 else dict()


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, alpha, n_iter, f32_input=False):
    x0 = noisy_square(shape)
    if f32_input:
        x0 = x0.astype(np.float32).astype(np.float64)
    return np_huber_cp(x0, n_iter, REG, alpha, scheme, _kw_of(shape))[:2]


def _solver(pytv, shape, dtype, scheme, alpha, **how):
    return pytv.solvers.HuberChambollePock(torch.as_tensor(noisy_square(shape).astype(dtype)).cuda(), REG, alpha, scheme=scheme, **_kw_of(shape),
                                           **how)


TRAJ_SHAPES = [(1, 1, 24, 28), (3, 2, 16, 20)]
STOP_SHAPES = [(1, 1, 32, 40), (3, 2, 16, 20)]


# ------------------------------------------------------------------------------------------------
# 5. solver trajectory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme, alpha):
    import pytv
    wx, wloss = np_trajectory(shape, scheme, alpha, 40)
    cp = _solver(pytv, shape, np.float64, scheme, alpha)
    assert cp.it == 0 and cp.gamma == 1.0 and cp.alpha == alpha and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape))
    assert (cp.tau, cp.sigma, cp.theta, cp.mu) == pytv.solvers.cp_linear_steps(cp.L2, 1.0, alpha / REG)
    np.testing.assert_allclose((cp.tau, cp.sigma, cp.theta), np_linear_steps(cp.L2, 1.0, alpha / REG), rtol=1e-14)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s alpha %g: loss rel %.3e  max|dx| %.3e" % (scheme, shape, alpha, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(noisy_square(shape))))
    assert cp.it == 40
    # run(15); run(25) is run(40) bit for bit
    two = _solver(pytv, shape, np.float64, scheme, alpha)
    np.testing.assert_array_equal(np.concatenate([two.run(15), two.run(25)]), loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.x_bar, cp.x_bar) and torch.equal(two.q, cp.q)
    # reset() reproduces the first run bit for bit; record_loss=False returns nothing and computes the same
    two.reset()
    assert two.it == 0 and torch.equal(two.x, two.x0) and torch.equal(two.x_bar, two.x0) and not bool(two.q.any())
    assert two.run(40, record_loss=False) is None
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.q, cp.q)
    two.reset()
    np.testing.assert_array_equal(two.run(40), loss)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme, alpha):
    """the fp32 tolerance of tests/test_gpu_cp_accel.py against the fp64 restatement on the fp32-rounded input: loss rtol 1e-5; result rtol
    1e-5, atol 2e-3"""
    import pytv
    wx, wloss = np_trajectory(shape, scheme, alpha, 40, f32_input=True)
    cp = _solver(pytv, shape, np.float32, scheme, alpha)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s alpha %g: loss rel %.3e  max|dx| %.3e" % (scheme, shape, alpha, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


def test_constructor_refuses_bad_alpha_and_gamma():
    import pytv
    x0 = torch.as_tensor(noisy_square((1, 1, 24, 28)).copy()).cuda()
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            pytv.solvers.HuberChambollePock(x0, REG, alpha)
    for gamma in (0.0, -0.5, 1.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            pytv.solvers.HuberChambollePock(x0, REG, 1.0, gamma=gamma)
    half = pytv.solvers.HuberChambollePock(x0, REG, 1.0, scheme="upwind", gamma=0.5)
    assert half.L2 == 8.0 and (half.tau, half.sigma, half.theta, half.mu) == pytv.solvers.cp_linear_steps(8.0, 0.5, 0.1)
    assert abs(half.tau * half.sigma * half.L2 - 1.0) <= 1e-15


# ------------------------------------------------------------------------------------------------
# 6. certified stop
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def np_x_star(shape, scheme, alpha):
    return np_huber_cp(noisy_square(shape), 2000, REG, alpha, scheme, _kw_of(shape))[0]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", STOP_SHAPES)
def test_run_until_certifies_where_the_restatement_does(shape, scheme, alpha):
    """NumPy restatement, iterations to a relative gap of 1e-6 checked every 10: 30 - 90 over these 16 cases"""
    import pytv
    kw = _kw_of(shape)
    want, wprimal, wgap = np_run_until(noisy_square(shape), 1e-6, 400, 10, REG, alpha, scheme, kw)
    assert 30 <= want <= 90
    cp = _solver(pytv, shape, np.float64, scheme, alpha)
    loss, info = cp.run_until(1e-6, 400, 10)
    dist = float(np.sqrt(np.sum((cp.result().cpu().numpy() - np_x_star(shape, scheme, alpha)) ** 2)))
    print("%s %s alpha %g: %r  restated: %d iterations, primal %.12e gap %.3e;  |x - x*| = %.3e" % (scheme, shape, alpha, info, want, wprimal, wgap,
                                                                                                  dist))
    assert info["converged"] is True and abs(info["iterations"] - want) <= 10 and len(loss) == info["iterations"] == cp.it
    assert 0.0 <= info["gap"] <= 1e-6 * info["primal"] and info["dual"] == info["primal"] - info["gap"]
    assert info["error_bound"] == np.sqrt(2 * info["gap"]) and info["error_bound"] >= dist
    if info["iterations"] == want:
        np.testing.assert_allclose(info["primal"], wprimal, rtol=1e-10)
        assert abs(info["gap"] - wgap) <= 1e-10 * wprimal
    # the certificate leaves the state of the loop alone
    state = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
    assert cp.duality_gap() == (info["primal"], info["dual"], info["gap"])
    assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q)))


# ------------------------------------------------------------------------------------------------
# 7. the rate: plain TV with the accelerated schedule is not there yet
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
@pytest.mark.parametrize("shape", STOP_SHAPES)
def test_accelerated_plain_tv_needs_more_iterations(shape, scheme, alpha):
    """NumPy first (tests/test_gpu_cp_accel.py's restatement of Algorithm 2 on plain TV, same data and weight): after the number of iterations
    at which the Huber model is certified to 1e-6 (40 - 90), the accelerated plain-TV loop has a relative gap of 1.2e-4 to 2.6e-3 in the 8
    cases -- none is a tie, so none is left out"""
    import pytv
    from test_gpu_cp_accel import np_accel, np_gap
    kw, x0 = _kw_of(shape), noisy_square(shape)
    n, _, _ = np_run_until(x0, 1e-6, 400, 10, REG, alpha, scheme, kw)
    ax, _, aq = np_accel(x0, n, REG, scheme, kw, want_q=True)
    wprimal, wgap = np_gap(ax, aq, x0, REG, scheme, kw)
    assert wgap > 1e-4 * wprimal                                        # the restatement separates the two by a factor of 100
    acc = pytv.solvers.AcceleratedChambollePock(torch.as_tensor(x0.copy()).cuda(), REG, scheme=scheme, **kw)
    acc.set_fused(False)
    acc.run(n)
    primal, _, gap = acc.duality_gap()
    hub = _solver(pytv, shape, np.float64, scheme, alpha)
    hub.run(n)
    hprimal, _, hgap = hub.duality_gap()
    print("%s %s alpha %g after %d iterations: relative gap Huber-TV %.3e, accelerated plain TV %.3e (restated %.3e)" % (
        scheme, shape, alpha, n, hgap / hprimal, gap / primal, wgap / wprimal))
    assert hgap <= 1e-6 * hprimal < 1e-6 * primal < gap


# ------------------------------------------------------------------------------------------------
# 8. front-end
# ------------------------------------------------------------------------------------------------
RAMP_SHAPE, RAMP_WEIGHT, RAMP_ALPHA = (24, 28), 10.0, 2.0


@functools.lru_cache(maxsize=None)
def noisy_ramp():
    """a linear ramp of 4 grey levels per column plus N(0, 3^2) noise"""
    ny, nx = RAMP_SHAPE
    clean = np.broadcast_to(4.0 * np.arange(nx, dtype=np.float64), (ny, nx)).copy()
    noisy = clean + 3.0 * np.random.default_rng(1).standard_normal((ny, nx))
    return clean, noisy


def flat_steps(u, tol=1e-3):
    """pairs of adjacent samples (along either axis) that are equal to ``tol``"""
    u = np.asarray(u, dtype=np.float64)
    return int(np.sum(np.abs(np.diff(u, axis=0)) <= tol) + np.sum(np.abs(np.diff(u, axis=1)) <= tol))


def test_denoise_tv_huber_front_end():
    import pytv
    shape = (1, 1, 24, 28)
    img = noisy_square(shape)[0, 0].astype(np.float32)
    vol = torch.as_tensor(img.reshape(shape)).cuda()
    # stops on run_until with its own check_every = 10
    out = pytv.denoise_tv_huber(img, 10.0, 2.0, rel_gap=1e-4, max_num_iter=200)
    ref = pytv.solvers.HuberChambollePock(vol, 10.0, 2.0, scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-4, 200, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] % 10 == 0 and info["iterations"] < 200
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == img.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # never converges: exactly 40 iterations, the solver's run(40)
    out = pytv.denoise_tv_huber(img, 10.0, 0.5, rel_gap=-1.0, max_num_iter=40, scheme="hybrid", check_every=20)
    ref = pytv.solvers.HuberChambollePock(vol, 10.0, 0.5, scheme="hybrid", reg_z_over_reg=1.0)
    ref.run(40)
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # torch in -> device tensor out; 3-D input; 4-D refused; alpha checked
    t = pytv.denoise_tv_huber(vol[0, 0], 10.0, 2.0)
    assert isinstance(t, torch.Tensor) and t.is_cuda and torch.equal(t.cpu(), torch.as_tensor(pytv.denoise_tv_huber(img, 10.0, 2.0)))
    stack = np.stack([img, img, img])
    assert pytv.denoise_tv_huber(stack, 10.0, 2.0, max_num_iter=10).shape == stack.shape
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.denoise_tv_huber(np.zeros((1, 1, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="alpha"):
        pytv.denoise_tv_huber(img, 10.0, 0.0)


def test_huber_tv_leaves_fewer_flat_steps_on_a_ramp_than_plain_tv():
    """NumPy figures (this file's restatement of Algorithm 3, 2000 iterations, against tests/test_gpu_cp_accel.py's plain-TV loop, 4000
    iterations; upwind, weight 10, alpha 2, the 24 x 28 ramp of ``noisy_ramp``): 1 flat step with Huber-TV against 118 with plain TV, of
    1292 pairs; mean absolute error to the clean ramp 1.462 against 1.568 (noisy: 2.288).  Weight 5 / alpha 2: 0 against 70; weight 20 /
    alpha 2: 1 against 232; weight 10 / alpha 4: 1 against 118."""
    import pytv
    clean, noisy = noisy_ramp()
    hub = pytv.denoise_tv_huber(noisy, RAMP_WEIGHT, RAMP_ALPHA, rel_gap=1e-9, max_num_iter=2000)
    tv = pytv.denoise_tv_chambolle(noisy, RAMP_WEIGHT, max_num_iter=4000, rel_gap=1e-9, accelerated=True)
    mae = lambda a: float(np.mean(np.abs(a - clean)))
    print("flat steps: Huber-TV %d, plain TV %d of %d pairs;  mean abs error to the clean ramp: noisy %.3f Huber-TV %.3f plain TV %.3f" % (
        flat_steps(hub), flat_steps(tv), 2 * clean.size - sum(RAMP_SHAPE), mae(noisy), mae(hub), mae(tv)))
    assert hub.dtype == np.float64 and flat_steps(hub) < flat_steps(tv)
