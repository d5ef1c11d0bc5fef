"""CPU-side checks of the Poisson / Kullback-Leibler Chambolle-Pock step: include/pytv4d.h declares tv_cp_primal_kl, the library exports it, the
ctypes table binds it, and every argument and halo error comes back before anything touches the device; the solver class and the front-end
exist with the documented signatures; tv_cp_primal_prox, its fidelity codes and the interface version are as they were.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

RESIDUAL = 1


def test_header_declares_library_exports_binding_binds_tv_cp_primal_kl():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_cp_primal_kl\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_cp_primal_kl"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const tv_geom* g", "const void* q", "const void* q_prev", "const void* q_next", "void* x", "void* x_bar", "const void* x0",
                      "double tau", "double theta", "int32_t flags", "double* out", "void* ws", "void* stream"]
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert re.search(r"^#define\s+TV_CPP_RESIDUAL\s+1\b", src, flags=re.M) and nv.TV_CPP_RESIDUAL == RESIDUAL
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_cp_primal_kl")
    res, args = nv._SIGNATURES["tv_cp_primal_kl"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
    assert [a is ctypes.c_int32 for a in args] == [p.startswith("int32_t ") for p in params]
    assert nv.lib().tv_cp_primal_kl.argtypes == args
    # the L2 / L1 / Huber entry point was not extended
    assert nv.FIDELITIES == {"l2": 0, "l1": 1, "huber": 2}
    assert not re.search(r"^#define\s+TV_FID_\w+\s+3\b", src, flags=re.M)


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed
Q = 8192


def _call(lib, g, **kw):
    a = dict(dict(q=P, qp=None, qn=None, x=P, x_bar=Q, x0=P, tau=0.3, theta=0.5, flags=0, out=P, ws=P), **kw)
    return lib.tv_cp_primal_kl(ctypes.byref(g) if g is not None else None, a["q"], a["qp"], a["qn"], a["x"], a["x_bar"], a["x0"], a["tau"],
                               a["theta"], a["flags"], a["out"], a["ws"], None)


def test_argument_errors_need_no_device():
    """an unknown flag bit, NULL g / arrays (x_bar in step mode only), x == x_bar, tau that is <= 0 or not finite, theta outside [0, 1] or not
    finite in step mode, and a tv_geom of another interface version return TV_E_ARG, each with its own text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for flags in (2, 3, 4, -2, 1 << 30):
                assert _call(lib, g, flags=flags) == -1, flags
                assert b"flag" in lib.tv_last_error()
            for flags in (0, RESIDUAL):
                for name in ("q", "x", "x0", "out", "ws") + (("x_bar",) if flags == 0 else ()):
                    assert _call(lib, g, flags=flags, **{name: None}) == -1, name
                    assert b"NULL" in lib.tv_last_error(), name
                assert _call(lib, g, flags=flags, x_bar=P) == -1
                assert b"x_bar" in lib.tv_last_error() and b"different" in lib.tv_last_error()
                for tau in (0.0, -0.25, float("nan"), float("inf"), float("-inf")):
                    assert _call(lib, g, flags=flags, tau=tau) == -1, tau
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
        assert _call(lib, g, flags=RESIDUAL, x_bar=None, theta=5.0) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert _call(lib, g, tau=-1.0) == -1 and _call(lib, g, theta=1.5) == -1 and _call(lib, g, x_bar=P) == -1 and _call(lib, g, flags=8) == -1
    assert _call(lib, g, x0=None) == -1


def test_solver_class_and_front_end_exist():
    import pytv
    cls = pytv.solvers.PoissonChambollePock
    assert issubclass(cls, pytv.solvers._ExtrapolatedCP) and "PoissonChambollePock" in pytv.solvers.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "scheme", "reg_z_over_reg", "reg_time", "mask_static", "factor_reg_static",
                                         "tau", "sigma", "slab", "pitch"]
    assert [init.parameters[k].default for k in list(init.parameters)[3:]] == ["hybrid", 1.0, 0.0, False, 0, None, None, None, "auto"]
    for name in ("step", "run", "run_steps", "result", "reset", "residuals", "initial_residual", "run_until"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_res", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert (cls.SLOTS, cls.F) == (pytv.solvers.ChambollePock.SLOTS, pytv.solvers.ChambollePock.F)
    doc = " ".join(cls.__doc__.split())
    for word in ("Kullback-Leibler", "one-sweep", "hipGraph", "persistent", "placement tuner"):          # the model, and what is not built
        assert word in doc, word
    assert "tv_cp_primal_kl" in cls.residuals.__doc__ and "tv_cp_primal_prox" in pytv.solvers.RobustChambollePock.residuals.__doc__
    # the residual plumbing is shared, not copied
    robust = pytv.solvers.RobustChambollePock
    for name in ("_residual_scalars", "_residual_dict", "initial_residual"):
        assert getattr(cls, name) is getattr(robust, name), name
    assert "PoissonChambollePock" in " ".join(robust.__doc__.split())
    sig = inspect.signature(pytv.denoise_tv_poisson)
    assert pytv.denoise_tv_poisson is pytv.restoration.denoise_tv_poisson and "denoise_tv_poisson" in pytv.__all__
    assert list(sig.parameters) == ["image", "weight", "rel_res", "max_num_iter", "scheme", "tau", "check_every"]
    assert [sig.parameters[k].default for k in sig.parameters][1:] == [1.0, 1e-2, 400, "upwind", None, 10]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("scheme", "tau", "check_every"))
    # the other front-ends are as they were
    assert list(inspect.signature(pytv.denoise_tv_robust).parameters) == ["image", "weight", "fidelity", "delta", "rel_res", "max_num_iter",
                                                                          "scheme", "tau", "check_every"]
