"""The optimality residual of the operator Chambolle-Pock solver on the GPU (``-m gpu``): tv_cp_dual_residual through the C-ABI against a NumPy
fp64 restatement (``orc.D`` and the projection formula, inputs up-cast for fp32), against what tv_cp_dual actually changes, at a fixed point,
on z-slabs cut by hand, on pitched arrays and weight maps; then ``ChambollePockOperator.residuals`` / ``run_until`` / ``norm_A``.

Tolerances: fp64 1e-12 against NumPy (a few hundred roundings of an fp64 sum), fp32 inputs with fp64 accumulation 2e-5 (the project's fp32 bar);
against tv_cp_dual 1e-13 in fp64 (the same site values, only the order of the fp64 sum differs)."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-12, np.float32: 2e-5}
DTYPES = [np.float64, np.float32]
SIGMA = 0.35


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def proj(v, lam):
    """projection of every site's channel vector onto the l2 ball of radius lam (README.md:149-151)"""
    return v / np.maximum(1.0, np.sqrt(np.sum(v * v, axis=1, keepdims=True)) / lam)


def ref_res(x, q, sigma, lam, scheme, kw):
    """(|D x|_{2,1}, sum_sites |q - proj(q + sigma D x)|^2 / sigma^2, share of the sites outside the ball before projection) in fp64"""
    x, q = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    Dx = orc.D(x, scheme, **kw)
    v = q + sigma * Dx
    outside = np.sqrt(np.sum(v * v, axis=1)) > lam
    return float(orc.compute_L21_norm(Dx)), float(np.sum((q - proj(v, lam)) ** 2) / sigma ** 2), float(np.mean(outside))


@functools.lru_cache(maxsize=None)
def make_inputs(shape, scheme, dtype, kwname="plain", seed=11):
    """random x and q, and the radius lam for which half the sites of q + sigma D x lie outside the ball: the median of their norms"""
    kw = _case_kw(kwname, shape)
    rng = np.random.default_rng(seed)
    x = (20.0 * rng.random(shape)).astype(dtype)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = (3.0 * rng.standard_normal((shape[0], nd) + tuple(shape[1:]))).astype(dtype)
    v = q.astype(np.float64) + SIGMA * orc.D(x.astype(np.float64), scheme, **kw)
    lam = float(np.median(np.sqrt(np.sum(v * v, axis=1))))
    return x, q, lam                                  # shared among the tests: nobody writes to them


def _case_kw(name, shape):
    rng = np.random.default_rng(17)
    if name == "time_factor":
        return dict(reg_z_over_reg=0.7, reg_time=0.5, mask_static=(0.25 + 2.0 * rng.random((1, 1) + tuple(shape[2:]))))
    if name == "weight_vol":
        return dict(reg_z_over_reg=0.7, reg_time=0.5, mask_static=(0.25 + 2.0 * rng.random(shape)))
    return dict(reg_time=0.5)


def _storage(t):
    """the whole allocation behind a (possibly pitched) view, pads included"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def gpu_res(x, q, sigma, lam, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None):
    """tv_cp_dual_residual on local planes [a, b) (whole volume by default); x and q live on the device as WHOLE arrays and the slab and its
    halo planes are pointers into them (dense) or copies with the geometry's pitches (pitched).  Returns the two scalars."""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    gkw = {k: (v[a:b] if (isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg and v.dtype != bool) else v) for k, v in kw.items()}
    g = nv.Geometry((b - a,) + tuple(x.shape[1:]), scheme, _tdt(dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1], **gkw)
    if pitch == (0, 0):
        xf, qf = torch.as_tensor(np.ascontiguousarray(x)).cuda(), torch.as_tensor(np.ascontiguousarray(q)).cuda()
        dev = dict(x=xf[a:b], q=qf[a:b], xp=xf[a - 1:a] if a > 0 else None, xn=xf[b:b + 1] if b < nzg else None)
        whole = dict(x=xf, q=qf)
    else:
        def put(t, arr):
            t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
            return t
        dev = dict(x=put(g.new_image(b - a), x[a:b]), q=put(g.new_grad(b - a), q[a:b]),
                   xp=put(g.new_image(1), x[a - 1:a]) if a > 0 else None, xn=put(g.new_image(1), x[b:b + 1]) if b < nzg else None)
        whole = {k: v for k, v in dev.items() if v is not None}
    before = {k: _storage(v).clone() for k, v in whole.items()}
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_dual_residual(g.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), float(sigma), float(lam),
                                          out.data_ptr(), nv.ptr(g.workspace()), nv.current_stream(g.device)))
    res = tuple(out.cpu().tolist())
    for k, t in whole.items():
        assert torch.equal(_storage(t), before[k]), "tv_cp_dual_residual wrote to " + k          # reduce-only: the whole allocation, pads included
    if keep is not None:
        keep.update(dev=dev, geom=g)
    return res


def close(got, ref, rtol, what=""):
    print("%s got %r ref %r  rel %s" % (what, tuple(got), tuple(ref), [abs(g - r) / abs(r) if r else abs(g) for g, r in zip(got, ref)]))
    for g, r in zip(got, ref):
        assert abs(g - r) <= rtol * abs(r), what


# ------------------------------------------------------------------------------------------------
# 1. the kernel against NumPy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(3, 2, 12, 20), (1, 1, 9, 13)])          # 16-byte lanes with z and time; odd nx: the scalar-lane form
def test_kernel_equals_numpy(shape, scheme, dtype):
    kw = _case_kw("plain", shape)
    x, q, lam = make_inputs(shape, scheme, dtype)
    tv, res, share = ref_res(x, q, SIGMA, lam, scheme, kw)
    assert 0.2 <= share <= 0.8                                              # both branches of the projection are taken
    assert res > 0
    close(gpu_res(x, q, SIGMA, lam, scheme, dtype, kw), (tv, res), RTOL[dtype], "%s %s" % (shape, scheme))


# ------------------------------------------------------------------------------------------------
# 2. it is what tv_cp_dual changes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(3, 2, 12, 20), (1, 1, 9, 13)])
def test_consistent_with_tv_cp_dual(shape, scheme, dtype):
    from pytv import _native as nv
    kw = _case_kw("plain", shape)
    x, q, lam = make_inputs(shape, scheme, dtype)
    keep = {}
    got = gpu_res(x, q, SIGMA, lam, scheme, dtype, kw, keep=keep)
    g, dev = keep["geom"], keep["dev"]
    q_new = dev["q"].clone()
    tv = torch.zeros((), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_dual(g.ref, nv.ptr(dev["x"]), None, None, nv.ptr(q_new), SIGMA, lam, tv.data_ptr(), nv.ptr(g.workspace()),
                                 nv.current_stream(g.device)))
    change = float(torch.sum((dev["q"].double() - q_new.double()) ** 2).item()) / SIGMA ** 2
    assert change > 0
    close(got, (float(tv.item()), change), 1e-13 if dtype == np.float64 else RTOL[dtype], "against tv_cp_dual %s %s" % (shape, scheme))


# ------------------------------------------------------------------------------------------------
# 3. zero at a fixed point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_zero_at_a_fixed_point(scheme, dtype):
    """x constant: D x = 0 exactly, and every q inside the ball is left alone.  q is feasible with room to spare (|q|_2 <= 0.9 lam, some sites
    0): ON the sphere "feasible" is a matter of the last bit of sqrt(sum q^2) / lam, which is not what this test is about."""
    shape, lam = (3, 2, 12, 20), 5.0
    kw = _case_kw("plain", shape)
    rng = np.random.default_rng(23)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = rng.standard_normal((shape[0], nd) + tuple(shape[1:]))
    q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True)) * (0.9 * lam * np.maximum(0.0, 1.5 * rng.random((shape[0], 1) + tuple(shape[1:])) - 0.5))
    q = q.astype(dtype)
    assert float(np.max(np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)))) <= 0.91 * lam and np.any(q != 0)
    x = np.full(shape, 37.25, dtype=dtype)
    assert gpu_res(x, q, SIGMA, lam, scheme, dtype, kw) == (0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# 4. slabs by hand
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["hybrid", "central"])
def test_slab_partials_add_up(scheme):
    shape, dtype = (6, 2, 12, 20), np.float64
    kw = _case_kw("plain", shape)
    x, q, lam = make_inputs(shape, scheme, dtype)
    whole = np.array(gpu_res(x, q, SIGMA, lam, scheme, dtype, kw))
    close(whole, ref_res(x, q, SIGMA, lam, scheme, kw)[:2], RTOL[dtype], "whole " + scheme)
    parts = sum(np.array(gpu_res(x, q, SIGMA, lam, scheme, dtype, kw, z_range=zr)) for zr in ((0, 2), (2, 5), (5, 6)))
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------
# 5. pitched arrays and weights
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_pitched_with_time_factor_equals_dense(scheme, dtype):
    shape, pitch = (3, 2, 5, 10), (12, 5 * 12 + 8)                          # row_pitch > nx: the last lane of a row holds pad columns (zeros)
    kw = _case_kw("time_factor", shape)
    x, q, lam = make_inputs(shape, scheme, dtype, "time_factor")
    dense = gpu_res(x, q, SIGMA, lam, scheme, dtype, kw)
    pitched = gpu_res(x, q, SIGMA, lam, scheme, dtype, kw, pitch=pitch)
    close(dense, ref_res(x, q, SIGMA, lam, scheme, kw)[:2], RTOL[dtype], "dense " + scheme)
    # the same sites through the 16-byte lanes instead of the scalar ones (nx = 10 is no multiple of a lane): fp64 sums of the same terms in
    # another order; the fp32 bar where the two instantiations may round a site's fp32 arithmetic differently
    close(pitched, dense, 1e-12 if dtype == np.float64 else RTOL[dtype], "pitched against dense " + scheme)


@pytest.mark.parametrize("dtype", DTYPES)
def test_time_weight_volume_equals_numpy(dtype):
    shape, scheme = (3, 3, 6, 8), "hybrid"
    kw = _case_kw("weight_vol", shape)
    x, q, lam = make_inputs(shape, scheme, dtype, "weight_vol")
    tv, res, share = ref_res(x, q, SIGMA, lam, scheme, kw)
    assert 0.2 <= share <= 0.8
    close(gpu_res(x, q, SIGMA, lam, scheme, dtype, kw), (tv, res), RTOL[dtype], "weight volume")
    parts = sum(np.array(gpu_res(x, q, SIGMA, lam, scheme, dtype, kw, z_range=zr)) for zr in ((0, 1), (1, 3)))
    close(parts, (tv, res), RTOL[dtype], "weight volume, two slabs")


# ------------------------------------------------------------------------------------------------
# 6. the solver
# ------------------------------------------------------------------------------------------------
SOLVER_KW = dict(reg_z_over_reg=1.0, reg_time=0.5)
LAM = 1.0


@functools.lru_cache(maxsize=None)
def problem(shape):
    """A = diag(a), a in {0, 1, 2, 3} (a mask and a scale: |A| = 3), b = A truth + noise, a random start"""
    rng = np.random.default_rng(7)
    a = np.array([0.0, 1.0, 2.0, 3.0])[rng.integers(0, 4, size=shape)]
    b = a * orc.phantom(shape, dtype=np.float64) + 0.5 * rng.standard_normal(shape)
    x_init = 50.0 * rng.random(shape)
    return a, b, x_init


def make_solver(pytv, shape, calls=None, **how):
    a, b, x_init = problem(shape)
    at = torch.as_tensor(a).cuda()

    def A(v):
        if calls is not None:
            calls["A"] += 1
        return at * v

    def AT(v):
        if calls is not None:
            calls["AT"] += 1
        return at * v

    return pytv.solvers.ChambollePockOperator(A, AT, torch.as_tensor(b).cuda(), torch.as_tensor(x_init).cuda(), LAM, scheme="hybrid", **SOLVER_KW, **how)


def ref_triple(cp, shape):
    """the residual of the solver's triple, restated in NumPy from its definition"""
    a, b, _ = problem(shape)
    x, p, q = (t.cpu().numpy().astype(np.float64) for t in (cp.x, cp.p, cp.q))
    Dx = orc.D(x, "hybrid", **SOLVER_KW)
    rx = float(np.sum((a * p + orc.D_T(q, "hybrid", **SOLVER_KW)) ** 2))
    rp = float(np.sum((p - (a * x - b)) ** 2))
    rq = float(np.sum((q - proj(q + cp.sigma_D * Dx, LAM)) ** 2) / cp.sigma_D ** 2)
    return {"x": rx, "p": rp, "q": rq, "total": rx + rp + rq, "tv": float(orc.compute_L21_norm(Dx)), "fid": float(0.5 * np.sum((a * x - b) ** 2))}


@pytest.mark.parametrize("way,shape,how", [("default", (2, 2, 16, 16), dict()), ("pair", (2, 2, 16, 16), dict(fused=False)),
                                           ("one_sweep", (2, 2, 16, 64), dict(fused=True))])
def test_solver_residuals_and_run_until(way, shape, how):
    import pytv
    from pytv import _native as nv
    if way == "one_sweep":
        g = nv.Geometry(shape, "hybrid", torch.float64, "cuda", **SOLVER_KW)
        if not nv.lib().tv_cp_fused_supported(g.ref):
            pytest.skip("tv_cp_fused_supported refuses %r: no one-sweep path to test" % (shape,))
    calls = {"A": 0, "AT": 0}
    cp = make_solver(pytv, shape, calls, norm_A=3.0, **how)
    assert cp.fused == (way == "one_sweep")
    assert cp.tau == 1.0 / (1.0 * 9.0 + 0.5 * 14.0)                       # L = 4 (2 + reg_z + reg_time) = 14
    assert (cp.n_A, cp.n_AT, cp.n_A_setup, cp.n_AT_setup) == (1, 0, 1, 0) and calls == {"A": 1, "AT": 0}
    done = 0
    for k in (0, 1, 5):
        if k > done:
            cp.run(k - done)
            done = k
        state = [t.clone() for t in (cp.x, cp.p, cp.q, cp.r)]
        counters = (cp.n_A, cp.n_AT, dict(calls))
        got = cp.residuals()
        assert all(torch.equal(s, t) for s, t in zip(state, (cp.x, cp.p, cp.q, cp.r)))          # bit-identical
        assert (cp.n_A, cp.n_AT, calls) == counters
        ref = ref_triple(cp, shape)
        print(way, "k =", k, got, ref)
        assert set(got) == {"x", "p", "q", "total", "tv", "fid"} and all(isinstance(v, float) for v in got.values())
        for key in ref:
            assert abs(got[key] - ref[key]) <= 1e-10 * abs(ref[key]), (k, key, got[key], ref[key])
        if k == 0:
            assert got["x"] == 0.0 and got["total"] == cp.initial_residual()
    r0 = cp.initial_residual()
    loss, info = cp.run_until(1e-3, 2000)
    print(way, {k: v for k, v in info.items() if k != "residuals"}, info["residuals"])
    assert info["converged"] is True and 0 < info["iterations"] <= 2000 and info["iterations"] % 10 == 0 and len(loss) == info["iterations"]
    assert info["initial"] == r0 and info["residuals"]["total"] <= 1e-6 * r0
    again = cp.residuals()
    assert again == info["residuals"] and again["total"] <= 1e-6 * r0
    n = done + info["iterations"]
    assert cp.n_A - cp.n_A_setup == n and cp.n_AT - cp.n_AT_setup == n                         # exactly one of each per iteration
    assert calls == {"A": 1 + n, "AT": n}


def test_run_until_returns_at_once_from_a_saddle_point():
    """x_init = 0, b = 0: the triple (0, 0, 0) is a saddle point, R_0 == 0"""
    import pytv
    shape = (2, 2, 16, 16)
    z = torch.zeros(shape, dtype=torch.float64, device="cuda")
    cp = pytv.solvers.ChambollePockOperator(lambda v: 3.0 * v, lambda v: 3.0 * v, z.clone(), z.clone(), LAM, scheme="hybrid", norm_A=3.0, **SOLVER_KW)
    loss, info = cp.run_until(1e-3, 100)
    assert info["converged"] is True and info["iterations"] == 0 and len(loss) == 0 and info["residuals"]["total"] == 0.0 and cp.n_AT == 0


# ------------------------------------------------------------------------------------------------
# 7. step safety
# ------------------------------------------------------------------------------------------------
def test_estimated_norm_gives_a_safe_step():
    """|A| = 3.  The default step of the parent commit for this case is tau = 1 / (1 + 14) = 0.0667, i.e. tau (sigma_A |A|^2 + sigma_D L) =
    16 / 15: just outside the condition (it assumes |A| <= 1); a projector with |A| in the tens is far outside.  Nothing here depends on
    that step blowing up."""
    import pytv
    shape = (2, 2, 16, 16)
    a, _, x_init = problem(shape)
    at = torch.as_tensor(a).cuda()
    est = pytv.solvers.operator_norm_sq(lambda v: at * v, lambda v: at * v, torch.as_tensor(x_init).cuda())
    print("operator_norm_sq", est)
    assert isinstance(est, float) and 9.0 <= est <= 9.0 * 1.06
    calls = {"A": 0, "AT": 0}
    cp = make_solver(pytv, shape, calls, norm_A="estimate")
    assert cp.norm_A_sq == est and cp.tau == 1.0 / (est + 0.5 * 14.0)
    assert (cp.n_A, cp.n_AT) == (21, 20) == (cp.n_A_setup, cp.n_AT_setup) and calls == {"A": 21, "AT": 20}     # counted
    loss = cp.run(200)
    assert np.all(np.isfinite(loss)) and np.all(np.diff(loss[-50:]) <= 0)
    assert cp.n_A - cp.n_A_setup == 200 and cp.n_AT - cp.n_AT_setup == 200
    explicit = make_solver(pytv, shape, norm_A="estimate", tau=0.01)
    assert explicit.tau == 0.01                                             # an explicit tau wins


# ------------------------------------------------------------------------------------------------
# 8. the default is unchanged, and asking does not disturb the loop
# ------------------------------------------------------------------------------------------------
def test_default_step_is_unchanged_and_residuals_do_not_disturb_the_loop():
    import pytv
    shape = (2, 2, 16, 16)
    plain, asked = make_solver(pytv, shape), make_solver(pytv, shape)
    assert plain.tau == pytv.solvers.cp_step_size(shape[0], shape[1], 1.0, 0.5) == 1.0 / 15.0 and plain.norm_A_sq is None
    want = plain.run(10)
    got = []
    for _ in range(10):
        asked.residuals()
        got.append(asked.run(1))
    assert torch.equal(asked.x, plain.x) and torch.equal(asked.q, plain.q) and torch.equal(asked.p, plain.p)
    np.testing.assert_array_equal(np.concatenate(got), want)
