"""CPU-side checks of the accelerated Chambolle-Pock solver: the step schedule (``pytv.solvers.accel_schedule``, a pure fp64 host function),
include/pytv4d.h declares tv_cp_primal_accel, the library exports it, the ctypes table binds it, and its argument and halo errors come back
before anything touches the device; the solver class and the front-end keyword exist.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


# ------------------------------------------------------------------------------------------------
# accel_schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau0,sigma0,gamma", [(8 ** -0.5, 8 ** -0.5, 1.0), (0.05, 2.5, 1.0), (0.3, 0.2, 0.35), (1.0, 1.0 / 12.0, 0.7)])
def test_schedule_keeps_the_product_and_theta_rises_inside_the_unit_interval(tau0, sigma0, gamma):
    from pytv.solvers import accel_schedule
    tau, sigma, theta = accel_schedule(tau0, sigma0, gamma, 3000)
    assert tau.dtype == sigma.dtype == theta.dtype == np.float64 and tau.shape == sigma.shape == theta.shape == (3000,)
    assert tau[0] == tau0 and sigma[0] == sigma0
    np.testing.assert_allclose(tau * sigma, tau0 * sigma0, rtol=1e-14, atol=0)
    assert np.all(theta > 0.0) and np.all(theta < 1.0) and np.all(np.diff(theta) > 0.0)
    # the recurrences themselves
    np.testing.assert_array_equal(theta, 1.0 / np.sqrt(1.0 + 2.0 * gamma * tau))
    np.testing.assert_array_equal(tau[1:], theta[:-1] * tau[:-1])
    np.testing.assert_allclose(sigma[1:], sigma[:-1] / theta[:-1], rtol=1e-14, atol=0)


def test_schedule_with_gamma_zero_is_constant():
    from pytv.solvers import accel_schedule
    tau, sigma, theta = accel_schedule(0.123, 0.77, 0.0, 500)
    assert np.all(tau == 0.123) and np.all(sigma == 0.77) and np.all(theta == 1.0)


def test_schedule_start_continues_bit_for_bit():
    from pytv.solvers import accel_schedule
    whole = accel_schedule(0.31, 0.4, 1.0, 400)
    for start, n in ((0, 400), (1, 10), (15, 25), (137, 263), (399, 1), (400, 0)):
        part = accel_schedule(0.31, 0.4, 1.0, n, start=start)
        for a, b in zip(part, whole):
            assert a.shape == (n,)
            np.testing.assert_array_equal(a, b[start:start + n])
    two = [np.concatenate(p) for p in zip(accel_schedule(0.31, 0.4, 1.0, 15), accel_schedule(0.31, 0.4, 1.0, 25, start=15))]
    for a, b in zip(two, accel_schedule(0.31, 0.4, 1.0, 40)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_schedule_asymptotic(gamma):
    """tau_k gamma k -> 1: the known asymptotic of Algorithm 2 (Chambolle & Pock 2011, Lemma 2 / Corollary 1)"""
    from pytv.solvers import accel_schedule
    k = 10000
    tau, _, _ = accel_schedule(8 ** -0.5, 8 ** -0.5, gamma, 1, start=k)
    assert abs(tau[0] * gamma * k - 1.0) <= 0.05


def test_schedule_refuses_bad_arguments():
    from pytv.solvers import accel_schedule
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, -0.1), (float("nan"), 1.0, 1.0), (1.0, float("inf"), 1.0)):
        with pytest.raises(ValueError):
            accel_schedule(*bad, 4)
    with pytest.raises(ValueError):
        accel_schedule(1.0, 1.0, 1.0, -1)
    with pytest.raises(ValueError):
        accel_schedule(1.0, 1.0, 1.0, 1, start=-1)


# ------------------------------------------------------------------------------------------------
# tv_cp_primal_accel: declaration, export, binding, argument checks
# ------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_binding_binds_tv_cp_primal_accel():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_cp_primal_accel\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_cp_primal_accel"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const tv_geom* g", "const void* q", "const void* q_prev", "const void* q_next", "void* x", "void* x_bar", "const void* x0",
                      "double tau", "double theta", "double* fid", "void* ws", "void* stream"]
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_cp_primal_accel")
    res, args = nv._SIGNATURES["tv_cp_primal_accel"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
    assert nv.lib().tv_cp_primal_accel.argtypes == args


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed
Q = 8192


def _call(lib, g, **kw):
    a = dict(dict(q=P, qp=None, qn=None, x=P, x_bar=Q, x0=P, tau=0.3, theta=0.5, fid=P, ws=P), **kw)
    return lib.tv_cp_primal_accel(ctypes.byref(g) if g is not None else None, a["q"], a["qp"], a["qn"], a["x"], a["x_bar"], a["x0"], a["tau"],
                                  a["theta"], a["fid"], a["ws"], None)


def test_argument_errors_need_no_device():
    """NULL g / arrays, x == x_bar, tau that is <= 0 or not finite, theta outside [0, 1] or not finite, and a tv_geom of another interface
    version return TV_E_ARG, each with its own text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for name in ("q", "x", "x_bar", "x0", "fid", "ws"):
                assert _call(lib, g, **{name: None}) == -1, name
                assert b"NULL" in lib.tv_last_error(), name
            assert _call(lib, g, x_bar=P) == -1
            assert b"x_bar" in lib.tv_last_error() and b"different" in lib.tv_last_error()
            for tau in (0.0, -0.25, float("nan"), float("inf"), float("-inf")):
                assert _call(lib, g, tau=tau) == -1, tau
                assert b"tau" in lib.tv_last_error() and b"theta" not in lib.tv_last_error()
            for theta in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf")):
                assert _call(lib, g, theta=theta) == -1, theta
                assert b"theta" in lib.tv_last_error()
    assert _call(lib, None) == -1
    assert b"tv_geom" in lib.tv_last_error()
    bad = _geom(nv)
    bad.abi_version = 4
    assert _call(lib, bad) == -1
    assert b"version" in lib.tv_last_error()


def test_missing_gradient_halo_on_a_sharded_geometry_is_TV_E_HALO():
    from pytv import _native as nv
    lib = nv.lib()
    for scheme in ("hybrid", "central"):                          # an interior slab: both gradient halo planes
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        assert _call(lib, g, qp=None, qn=P) == -2 and b"halo" in lib.tv_last_error()
        assert _call(lib, g, qp=P, qn=None) == -2 and b"halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # the adjoint of a forward difference looks backwards, of a backward one forwards
    assert _call(lib, up, qp=None, qn=P) == -2
    down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
    assert _call(lib, down, qp=P, qn=None) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert _call(lib, g, tau=-1.0) == -1 and _call(lib, g, theta=1.5) == -1 and _call(lib, g, x_bar=P) == -1


# ------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------
def test_solver_class_and_front_end_keyword_exist():
    import pytv
    cls = pytv.solvers.AcceleratedChambollePock
    assert issubclass(cls, pytv.solvers._SlabProblem)
    assert "AcceleratedChambollePock" in pytv.solvers.__all__ and "accel_schedule" in pytv.solvers.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "scheme", "reg_z_over_reg", "reg_time", "mask_static", "factor_reg_static", "tau0",
                                         "sigma0", "gamma", "slab", "pitch"]
    assert init.parameters["tau0"].default is None and init.parameters["sigma0"].default is None and init.parameters["gamma"].default == 1.0
    assert init.parameters["scheme"].default == "hybrid" and init.parameters["pitch"].default == "auto"
    for name in ("step", "run", "run_steps", "result", "duality_gap", "run_until", "reset"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_gap", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    doc = " ".join(cls.run.__doc__.split())
    assert "progress indicator" in doc and "duality_gap()[0]" in doc          # what the loss history is, and where the exact value is
    assert (cls.SLOTS, cls.F) == (pytv.solvers.ChambollePock.SLOTS, pytv.solvers.ChambollePock.F)
    sig = inspect.signature(pytv.denoise_tv_chambolle)
    assert sig.parameters["accelerated"].default is False and sig.parameters["accelerated"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(pytv.solvers.accel_schedule).parameters) == ["tau0", "sigma0", "gamma", "n", "start"]
    assert inspect.signature(pytv.solvers.accel_schedule).parameters["start"].default == 0
