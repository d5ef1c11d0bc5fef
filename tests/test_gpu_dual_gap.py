"""The duality-gap certificate on the GPU (``-m gpu``): tv_dual_gap through the C-ABI against the fp64 oracle (``orc.D``, ``orc.D_T`` on the
same inputs, up-cast for fp32, the gap summed in its site-wise form), the plane-marching form against the one-site form, z-slabs against the
whole volume, "nothing is written", and ``duality_gap`` / ``run_until`` of the solvers and the front-end.

Tolerances: out[0] = |D x|_{2,1} and out[1] = 1/2 |x - x0|^2 to the project's rtol (tests/test_gpu_parity.py: 1e-5 fp32, 1e-11 fp64);
out[2], the gap: |got - ref| <= rtol * ref + 16 eps_dtype P_ref -- the second term is the cancellation floor of lambda |D x| - <q, D x>
(a handful of roundings of terms of size lambda |D x|), which matters only for the converged states of the solver tests."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
DTYPES = [np.float64, np.float32]


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def ref_gap(x, q, x0, lam, qscale, scheme, kw):
    """(|D x|_{2,1}, 1/2 |x - x0|^2, gap) in fp64 with the gap in its site-wise form"""
    x, q, x0 = (np.asarray(a, dtype=np.float64) for a in (x, q, x0))
    Dx = orc.D(x, scheme, **kw)
    qs = qscale * q
    gd = orc.D_T(qs, scheme, **kw)
    nrm = np.sqrt(np.sum(Dx * Dx, axis=1))
    gap = np.sum(0.5 * (x - x0 + gd) ** 2) + np.sum(lam * nrm - np.sum(qs * Dx, axis=1))
    return float(orc.compute_L21_norm(Dx)), float(0.5 * np.sum((x - x0) ** 2)), float(gap)


def check(got, ref, lam, dtype, what=""):
    rtol, eps = RTOL[dtype], float(np.finfo(dtype).eps)
    P = ref[1] + lam * ref[0]
    print("%s got %r ref %r  P %.6e  |d gap| %.3e" % (what, tuple(got), ref, P, abs(got[2] - ref[2])))
    assert abs(got[0] - ref[0]) <= rtol * abs(ref[0]), what
    assert abs(got[1] - ref[1]) <= rtol * abs(ref[1]), what
    assert abs(got[2] - ref[2]) <= rtol * abs(ref[2]) + 16 * eps * P, what


def feasible_q(rng, shape_grad, radius, dtype):
    """random dual variable with per-site |q|_2 <= radius: some sites on the sphere, the others inside"""
    q = rng.standard_normal(shape_grad)
    n = np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    r = np.minimum(1.0, 1.5 * rng.random(n.shape))
    return (q / np.maximum(n, 1e-30) * (radius * r)).astype(dtype)


def make_inputs(shape, scheme, dtype, kw, lam, qscale, seed=5):
    rng = np.random.default_rng(seed)
    x = (60.0 * rng.random(shape)).astype(dtype)
    x0 = (60.0 * rng.random(shape)).astype(dtype)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = feasible_q(rng, (shape[0], nd) + tuple(shape[1:]), lam / qscale, dtype)
    return x, q, x0


def _z_channels(scheme):
    per = 2 if scheme == "hybrid" else 1
    return 2 * per, 2 * per + (1 if scheme == "hybrid" else 0)        # (adjoint looks backwards, forwards): pytv/slab.py HaloPlan


def gpu_gap(x, q, x0, lam, qscale, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None):
    """tv_dual_gap on local planes [a, b) of the arrays (whole volume by default), halo planes passed by hand; returns the three scalars"""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = nv.Geometry((b - a,) + tuple(x.shape[1:]), scheme, _tdt(dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1],
                    **({k: (v[a:b] if (isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg and v.dtype != bool) else v) for k, v in kw.items()}))

    def img(arr):
        t = g.new_image(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    def grad(arr):
        t = g.new_grad(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), q=grad(q[a:b]), x0=img(x0[a:b]),
               xp=img(x[a - 1:a]) if a > 0 else None, xn=img(x[b:b + 1]) if b < nzg else None,
               qp=img(q[a - 1:a, cb]) if (a > 0 and g.z_active) else None, qn=img(q[b:b + 1, cf]) if (b < nzg and g.z_active) else None)
    before = {k: _storage(v).clone() for k, v in dev.items() if v is not None}
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_dual_gap(g.ref, nv.ptr(dev["x"]), nv.ptr(dev["xp"]), nv.ptr(dev["xn"]), nv.ptr(dev["q"]), nv.ptr(dev["qp"]), nv.ptr(dev["qn"]),
                                  nv.ptr(dev["x0"]), float(lam), float(qscale), out.data_ptr(), nv.ptr(g.workspace()), nv.current_stream(g.device)))
    res = tuple(out.cpu().tolist())
    if keep is not None:
        keep.update(dev=dev, before=before)
    return res


def _storage(t):
    """the whole allocation behind a (possibly pitched) view, pads included"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


# ------------------------------------------------------------------------------------------------
# 1. parity through the C-ABI
# ------------------------------------------------------------------------------------------------
def _case_kw(name, shape):
    rng = np.random.default_rng(17)
    if name == "mask":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=rng.random((1, 1) + shape[2:]) < 0.4, factor_reg_static=3.0)
    if name == "time_factor":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random((1, 1) + shape[2:])))
    if name == "weight_vol":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random(shape)))
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


CASES = [("vector_rows", (3, 2, 5, 8), (0, 0)), ("scalar_rows", (3, 2, 6, 7), (0, 0)), ("no_z_no_time", (1, 1, 9, 12), (0, 0)),
         ("two_point_time", (4, 2, 5, 8), (0, 0)), ("mask", (2, 3, 5, 8), (0, 0)), ("time_factor", (2, 3, 5, 8), (0, 0)),
         ("weight_vol", (2, 3, 5, 8), (0, 0)), ("pitched", (3, 2, 5, 10), (12, 5 * 12 + 8))]


# (the two-point time axis that falls back to the forward stencil is a case of the central scheme only)
CASE_SCHEMES = [(n, sh, pt, sc) for n, sh, pt in CASES for sc in SCHEMES if n != "two_point_time" or sc == "central"]


@pytest.mark.parametrize("qscale", [1.0, 2.5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,shape,pitch,scheme", CASE_SCHEMES)
def test_parity_with_the_oracle(name, shape, pitch, scheme, dtype, qscale):
    lam = 5.0
    kw = _case_kw(name, shape)
    x, q, x0 = make_inputs(shape, scheme, dtype, kw, lam, qscale)
    got = gpu_gap(x, q, x0, lam, qscale, scheme, dtype, kw, pitch=pitch)
    ref = ref_gap(x, q, x0, lam, qscale, scheme, kw)
    assert ref[2] > 0.1 * (ref[1] + lam * ref[0])                  # an unconverged pair: the gap is large
    check(got, ref, lam, dtype, "%s %s" % (name, scheme))


# ------------------------------------------------------------------------------------------------
# 2. plane-marching form (fp32, planes of >= 4 MiB): two launches, against the one-site form and the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,shape", [("hybrid", (3, 1, 1024, 1024)), ("upwind", (3, 1, 1024, 1024)), ("downwind", (3, 1, 1024, 1024)),
                                          ("central", (2, 2, 1024, 1024))])
def test_marching_form_equals_one_site_form_and_oracle(scheme, shape, tvopt):
    lam, dtype = 5.0, np.float32
    kw = dict(reg_z_over_reg=0.7, reg_time=0.25)
    x, q, x0 = make_inputs(shape, scheme, dtype, kw, lam, 1.0)
    ref = ref_gap(x, q, x0, lam, 1.0, scheme, kw)
    march = gpu_gap(x, q, x0, lam, 1.0, scheme, dtype, kw)
    tvopt("TV_NO_MARCH", 1)
    site = gpu_gap(x, q, x0, lam, 1.0, scheme, dtype, kw)
    check(march, ref, lam, dtype, "marching " + scheme)
    check(site, ref, lam, dtype, "one-site " + scheme)
    check(march, site, lam, dtype, "marching against one-site " + scheme)


# ------------------------------------------------------------------------------------------------
# 3. slabs: the partial scalars add up to the whole-volume call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(6, 2, 5, 8), (5, 1, 6, 132)])
def test_slab_partials_add_up(shape, scheme, dtype):
    lam = 5.0
    kw = dict(reg_z_over_reg=0.7, reg_time=0.25)
    x, q, x0 = make_inputs(shape, scheme, dtype, kw, lam, 1.0)
    whole = np.array(gpu_gap(x, q, x0, lam, 1.0, scheme, dtype, kw))
    check(whole, ref_gap(x, q, x0, lam, 1.0, scheme, kw), lam, dtype, "whole")
    nz = shape[0]
    cuts = [(0, c, nz) for c in range(1, nz)] + [(0, 1, nz - 2, nz)]
    tol = 1e-12 if dtype == np.float64 else 1e-6
    for cut in cuts:
        parts = sum(np.array(gpu_gap(x, q, x0, lam, 1.0, scheme, dtype, kw, z_range=(a, b))) for a, b in zip(cut[:-1], cut[1:]))
        np.testing.assert_allclose(parts, whole, rtol=tol, atol=0, err_msg="cut %r" % (cut,))


# ------------------------------------------------------------------------------------------------
# 4. nothing is written
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_inputs_are_left_bit_identical(scheme, dtype):
    lam = 5.0
    kw = dict(reg_z_over_reg=0.7, reg_time=0.25)
    shape, pitch = (4, 2, 5, 10), (12, 5 * 12 + 8)
    x, q, x0 = make_inputs(shape, scheme, dtype, kw, lam, 1.0)
    for pt, zr in ((pitch, None), ((0, 0), (1, 3)), (pitch, (1, 3))):
        keep = {}
        gpu_gap(x, q, x0, lam, 1.0, scheme, dtype, kw, pitch=pt, z_range=zr, keep=keep)
        for k, t in keep["dev"].items():
            if t is not None:
                assert torch.equal(_storage(t), keep["before"][k]), k          # the whole allocation: pad columns included
        if pt != (0, 0):
            xs = keep["dev"]["x"]
            pads = _storage(xs).clone()
            pads.as_strided(xs.shape, xs.stride()).zero_()
            assert not bool(pads.any())                                        # what is not a voxel is a pad, and it is still zero


# ------------------------------------------------------------------------------------------------
# 5. solver level
# ------------------------------------------------------------------------------------------------
SOLVER_KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
LAM = 5.0


@functools.lru_cache(maxsize=None)
def noisy(shape, dtype):
    rng = np.random.default_rng(3)
    return (orc.phantom(shape, dtype=np.float64) + 10.0 * rng.standard_normal(shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def x_star(shape, scheme):
    """the oracle's 3000-iteration Chambolle-Pock iterate: the minimiser to ~1e-12 of the objective"""
    return orc.chambolle_pock(noisy(shape, np.float64), 3000, LAM, scheme=scheme, **SOLVER_KW)[0]


def _cp(pytv, shape, dtype, scheme, **how):
    return pytv.solvers.ChambollePock(torch.as_tensor(noisy(shape, dtype)).cuda(), LAM, scheme=scheme, **SOLVER_KW, **how)


# (the one-sweep kernel is fp32 only)
WAYS = [("persistent", (3, 2, 12, 16), dict(persistent=True), np.float64), ("persistent", (3, 2, 12, 16), dict(persistent=True), np.float32),
        ("pair", (3, 2, 12, 16), dict(fused=False, persistent=False), np.float64), ("pair", (3, 2, 12, 16), dict(fused=False, persistent=False), np.float32),
        ("one_sweep", (8, 1, 8, 64), dict(fused=True), np.float32)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("way,shape,how,dtype", WAYS)
def test_cp_duality_gap_matches_oracle_and_leaves_the_state(way, shape, how, dtype, scheme, tvopt):
    import pytv
    if way == "one_sweep":
        tvopt("TV_FUSED_MIN_KVOXELS", 0)
    cp, twin = _cp(pytv, shape, dtype, scheme, **how), _cp(pytv, shape, dtype, scheme, **how)
    assert (cp.small, cp.fused) == (way == "persistent", way == "one_sweep")
    cp.run(50)
    twin.run(50)
    primal, dual, gap = cp.duality_gap()
    x, q = cp.result().cpu().numpy(), cp.q.cpu().numpy()
    ref = ref_gap(x, q, noisy(shape, dtype), LAM, 1.0, scheme, SOLVER_KW)
    P = ref[1] + LAM * ref[0]
    check((ref[0], ref[1], gap), ref, LAM, dtype, "%s %s gap" % (way, scheme))
    assert abs(primal - P) <= RTOL[dtype] * P and abs((primal - dual) - gap) <= 1e-12 * primal
    assert float(np.max(np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)))) <= LAM * (1 + 4 * np.finfo(dtype).eps)       # q is feasible
    print("gap / primal after 50 iterations: %.3e" % (gap / primal))
    assert gap >= 0 and gap / primal < 1e-2
    assert cp.duality_gap() == (primal, dual, gap)                                   # asking twice changes nothing
    np.testing.assert_array_equal(cp.run(10), twin.run(10))                          # ... and neither does it disturb the loop


@pytest.mark.parametrize("scheme", SCHEMES)
def test_cp_run_until_certifies_the_distance_to_the_minimiser(scheme):
    import pytv
    shape = (3, 2, 12, 16)
    cp = _cp(pytv, shape, np.float64, scheme)
    loss, info = cp.run_until(1e-4, 2000)
    print(scheme, info)
    assert info["converged"] and info["iterations"] <= 800 and info["iterations"] % 10 == 0 and len(loss) == info["iterations"]
    assert info["gap"] <= 1e-4 * info["primal"] and abs(info["primal"] - info["dual"] - info["gap"]) <= 1e-12 * info["primal"]
    assert info["error_bound"] == np.sqrt(2 * info["gap"])
    dist2 = 0.5 * float(np.sum((cp.result().cpu().numpy() - x_star(shape, scheme)) ** 2))
    print("1/2 |x - x*|^2 = %.6e <= gap = %.6e" % (dist2, info["gap"]))
    assert dist2 <= info["gap"]
    assert cp.it == info["iterations"]


def test_cp_run_until_ends_on_the_iteration_limit_below_the_fp32_floor():
    import pytv
    cp = _cp(pytv, (3, 2, 12, 16), np.float32, "hybrid")
    loss, info = cp.run_until(1e-12, 40)
    assert info["converged"] is False and info["iterations"] == 40 and len(loss) == 40
    assert info["error_bound"] == float(np.sqrt(2.0 * max(info["gap"], 0.0)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("persistent", [False, True])
def test_admm_duality_gap_and_run_until(persistent, scheme, dtype):
    import pytv
    shape, rho = (3, 2, 12, 16), 2.0
    ad = pytv.solvers.ADMM(torch.as_tensor(noisy(shape, dtype)).cuda(), LAM, rho, n_cg=10, scheme=scheme, x_solver="chebyshev",
                           persistent=persistent, **SOLVER_KW)
    assert ad.cheb and ad.small == persistent
    ad.run(20)
    primal, dual, gap = ad.duality_gap()
    x, u = ad.result().cpu().numpy(), ad.u.cpu().numpy()
    ref = ref_gap(x, u, noisy(shape, dtype), LAM, rho, scheme, SOLVER_KW)
    check((ref[0], ref[1], gap), ref, LAM, dtype, "admm %s" % scheme)
    assert abs(primal - (ref[1] + LAM * ref[0])) <= RTOL[dtype] * primal
    loss, info = ad.run_until(1e-4, 200)
    print(scheme, info)
    assert info["converged"] and info["iterations"] <= 200 and info["iterations"] % 5 == 0 and info["gap"] <= 1e-4 * info["primal"]


def test_denoise_tv_chambolle_rel_gap_and_unchanged_default():
    import pytv
    img = np.load(os.path.join(GOLDEN, "cameraman.npz"))["image"].astype(np.float64) / 255.0
    rng = np.random.default_rng(0)
    noisy_img = img + 0.1 * rng.standard_normal(img.shape)
    weight = 0.1
    out = pytv.denoise_tv_chambolle(noisy_img, weight, rel_gap=1e-4, max_num_iter=2000)
    ref = pytv.solvers.ChambollePock(torch.as_tensor(noisy_img.reshape(1, 1, *img.shape)).cuda(), weight, scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-4, 2000)
    print(info)
    assert info["converged"] and info["iterations"] < 2000                       # stops before max_num_iter ...
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))     # ... and the front-end is that loop
    # the default: the loop the front-end has always run (objective moved by less than eps over ten iterations), bit for bit
    cp = pytv.solvers.ChambollePock(torch.as_tensor(noisy_img.reshape(1, 1, *img.shape)).cuda(), weight, scheme="upwind", reg_z_over_reg=1.0)
    prev, done = None, 0
    while done < 200:
        e = float(cp.run(10)[-1])
        done += 10
        if prev is not None and abs(prev - e) <= 2.0e-4 * max(abs(prev), 1e-30):
            break
        prev = e
    want = cp.result().cpu().numpy().reshape(img.shape)
    np.testing.assert_array_equal(pytv.denoise_tv_chambolle(noisy_img, weight), want)
    np.testing.assert_array_equal(pytv.denoise_tv_chambolle(noisy_img, weight, rel_gap=None), want)


# ------------------------------------------------------------------------------------------------
# 6. sharded solver: 2 ranks on one GPU over gloo
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, shape, dtype_name, ret):
    import torch.distributed as dist
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pytv
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(shape[0])
        x0 = torch.as_tensor(slab.local(noisy(shape, np.dtype(dtype_name).type)).copy()).cuda()
        cp = pytv.solvers.ChambollePock(x0, LAM, scheme="hybrid", slab=slab, **SOLVER_KW)
        cp.run(20)
        first = cp.duality_gap()
        again = cp.duality_gap()
        ret[rank] = (first, again, cp.fused)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_duality_gap_equals_unsharded(dtype, tvopt):
    import pytv
    import torch.multiprocessing as mp
    tvopt("TV_FUSED_MIN_KVOXELS", 0)
    shape = (8, 3, 6, 132)
    ret = mp.Manager().dict()
    mp.spawn(_rank, args=(2, _free_port(), shape, np.dtype(dtype).name, ret), nprocs=2, join=True)
    cp = pytv.solvers.ChambollePock(torch.as_tensor(noisy(shape, dtype)).cuda(), LAM, scheme="hybrid", **SOLVER_KW)
    cp.run(20)
    want = cp.duality_gap()
    print("unsharded", want, "ranks", dict(ret))
    assert ret[0][0] == ret[1][0] and ret[0][0] == ret[0][1]                     # every rank the same three numbers, asking again too
    assert ret[0][2] == cp.fused
    np.testing.assert_allclose(ret[0][0], want, rtol=1e-12 if dtype == np.float64 else 1e-6, atol=0)
