"""CPU-side checks of the robust-fidelity Chambolle-Pock step: include/pytv4d.h declares tv_cp_primal_prox and its constants, the library
exports it, the ctypes table binds it, and every argument and halo error comes back before anything touches the device; the solver class and
the front-end exist with the documented signatures.  No GPU."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

L2, L1, HUBER, RESIDUAL = 0, 1, 2, 1


def test_header_declares_library_exports_binding_binds_tv_cp_primal_prox():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    for name, val in (("TV_FID_L2", L2), ("TV_FID_L1", L1), ("TV_FID_HUBER", HUBER), ("TV_CPP_RESIDUAL", RESIDUAL)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, val), src, flags=re.M), name
    assert nv.FIDELITIES == {"l2": L2, "l1": L1, "huber": HUBER} and nv.TV_CPP_RESIDUAL == RESIDUAL
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_cp_primal_prox\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_cp_primal_prox"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const tv_geom* g", "const void* q", "const void* q_prev", "const void* q_next", "void* x", "void* x_bar", "const void* x0",
                      "int32_t fidelity", "double delta", "double tau", "double theta", "int32_t flags", "double* out", "void* ws", "void* stream"]
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_cp_primal_prox")
    res, args = nv._SIGNATURES["tv_cp_primal_prox"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
    assert [a is ctypes.c_int32 for a in args] == [p.startswith("int32_t ") for p in params]
    assert nv.lib().tv_cp_primal_prox.argtypes == args


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed
Q = 8192


def _call(lib, g, **kw):
    a = dict(dict(q=P, qp=None, qn=None, x=P, x_bar=Q, x0=P, fidelity=L1, delta=0.5, tau=0.3, theta=0.5, flags=0, out=P, ws=P), **kw)
    return lib.tv_cp_primal_prox(ctypes.byref(g) if g is not None else None, a["q"], a["qp"], a["qn"], a["x"], a["x_bar"], a["x0"], a["fidelity"],
                                 a["delta"], a["tau"], a["theta"], a["flags"], a["out"], a["ws"], None)


def test_argument_errors_need_no_device():
    """an unknown fidelity or flag bit, NULL g / arrays (x_bar in step mode only), x == x_bar, tau that is <= 0 or not finite, a Huber delta that
    is <= 0 or not finite, theta outside [0, 1] or not finite in step mode, and a tv_geom of another interface version return TV_E_ARG, each
    with its own text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for fidelity in (-1, 3, 17):
                assert _call(lib, g, fidelity=fidelity) == -1, fidelity
                assert b"fidelity" in lib.tv_last_error()
            for flags in (2, 3, 4, -2, 1 << 30):
                assert _call(lib, g, flags=flags) == -1, flags
                assert b"flag" in lib.tv_last_error()
            for flags in (0, RESIDUAL):
                for name in ("q", "x", "x0", "out", "ws") + (("x_bar",) if flags == 0 else ()):
                    assert _call(lib, g, flags=flags, **{name: None}) == -1, name
                    assert b"NULL" in lib.tv_last_error(), name
                assert _call(lib, g, flags=flags, x_bar=P) == -1
                assert b"x_bar" in lib.tv_last_error() and b"different" in lib.tv_last_error()
                for fidelity in (L2, L1, HUBER):
                    for tau in (0.0, -0.25, float("nan"), float("inf"), float("-inf")):
                        assert _call(lib, g, flags=flags, fidelity=fidelity, tau=tau) == -1, tau
                        assert b"tau" in lib.tv_last_error() and b"theta" not in lib.tv_last_error()
                for delta in (0.0, -1.0, float("nan"), float("inf")):
                    assert _call(lib, g, flags=flags, fidelity=HUBER, delta=delta) == -1, delta
                    assert b"delta" in lib.tv_last_error()
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
    """(with every argument valid the halo check is the last one before the launch: these calls return without following a pointer)"""
    from pytv import _native as nv
    lib = nv.lib()
    for flags in (0, RESIDUAL):
        for scheme in ("hybrid", "central"):                          # an interior slab: both gradient halo planes
            g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
            assert _call(lib, g, flags=flags, qp=None, qn=P) == -2 and b"halo" in lib.tv_last_error()
            assert _call(lib, g, flags=flags, qp=P, qn=None) == -2 and b"halo" in lib.tv_last_error()
        up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # the adjoint of a forward difference looks backwards, of a backward one forwards
        assert _call(lib, up, flags=flags, qp=None, qn=P) == -2
        down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
        assert _call(lib, down, flags=flags, qp=P, qn=None) == -2
        # residual mode: x_bar = NULL is no error (the halo error is reached), and neither is any theta
        assert _call(lib, g, flags=RESIDUAL, x_bar=None, theta=float("nan")) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert _call(lib, g, tau=-1.0) == -1 and _call(lib, g, theta=1.5) == -1 and _call(lib, g, x_bar=P) == -1
    assert _call(lib, g, fidelity=5) == -1 and _call(lib, g, flags=8) == -1 and _call(lib, g, fidelity=HUBER, delta=0.0) == -1
    # delta is read for Huber only
    assert _call(lib, g, fidelity=L1, delta=float("nan")) == -2 and _call(lib, g, fidelity=L2, delta=-1.0) == -2


def test_solver_class_and_front_end_exist():
    import pytv
    cls = pytv.solvers.RobustChambollePock
    assert issubclass(cls, pytv.solvers._SlabProblem) and "RobustChambollePock" in pytv.solvers.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "fidelity", "delta", "scheme", "reg_z_over_reg", "reg_time", "mask_static",
                                         "factor_reg_static", "tau", "sigma", "slab", "pitch"]
    assert init.parameters["fidelity"].default == "l1" and init.parameters["delta"].default is None
    assert init.parameters["tau"].default is None and init.parameters["sigma"].default is None
    assert init.parameters["scheme"].default == "hybrid" and init.parameters["pitch"].default == "auto"
    for name in ("step", "run", "run_steps", "result", "reset", "residuals", "initial_residual", "run_until"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_res", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert (cls.SLOTS, cls.F) == (pytv.solvers.ChambollePock.SLOTS, pytv.solvers.ChambollePock.F)
    doc = " ".join(cls.__doc__.split())
    assert "few grey levels" in doc and "tau = 5" in doc                                   # the advice on the step
    for word in ("one-sweep", "hipGraph", "persistent", "placement tuner", "Poisson"):       # what is out of scope
        assert word in doc, word
    sig = inspect.signature(pytv.denoise_tv_robust)
    assert pytv.denoise_tv_robust is pytv.restoration.denoise_tv_robust
    assert list(sig.parameters) == ["image", "weight", "fidelity", "delta", "rel_res", "max_num_iter", "scheme", "tau", "check_every"]
    assert [sig.parameters[k].default for k in sig.parameters][1:] == [1.0, "l1", None, 1e-2, 400, "upwind", None, 10]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("scheme", "tau", "check_every"))
    # denoise_tv_chambolle is as it was
    assert list(inspect.signature(pytv.denoise_tv_chambolle).parameters) == ["image", "weight", "eps", "max_num_iter", "scheme", "check_every",
                                                                             "rel_gap", "accelerated"]
