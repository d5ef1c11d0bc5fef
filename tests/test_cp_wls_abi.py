"""CPU-side checks of the weighted least-squares / box Chambolle-Pock step: include/pytv4d.h declares tv_cp_primal_wls, the library exports it,
the ctypes table binds it, and every argument and halo error comes back before anything touches the device (the pointers passed are never
followed); the solver class and the front-end exist with the documented signatures; the interface version is as it was.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

RESIDUAL = 1
PARAMS = ["const tv_geom* g", "const void* q", "const void* q_prev", "const void* q_next", "void* x", "void* x_bar", "const void* x0",
          "const void* w", "double lo", "double hi", "double tau", "double theta", "int32_t flags", "double* out", "void* ws", "void* stream"]


def test_header_declares_library_exports_binding_binds_tv_cp_primal_wls():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_cp_primal_wls\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_cp_primal_wls"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == PARAMS
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_cp_primal_wls")
    res, args = nv._SIGNATURES["tv_cp_primal_wls"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
    assert [a is ctypes.c_int32 for a in args] == [p.startswith("int32_t ") for p in params]
    assert nv.lib().tv_cp_primal_wls.argtypes == args
    assert nv.lib().tv_abi_version() == 5 == nv.ABI_VERSION
    # the header says why the box must contain 0, and who shifts the problem
    doc = " ".join(re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+tv_cp_primal_wls", src, flags=re.S).group(1).split())
    for word in ("pad", "contain 0", "shift", "WeightedChambollePock", "Nd + 5", "Nd + 3", "BIT FOR BIT"):
        assert word in doc, word
    # the neighbouring entry points were not extended
    assert len(nv._SIGNATURES["tv_cp_primal_kl"][1]) == 13 and len(nv._SIGNATURES["tv_cp_primal_prox"][1]) == 15


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed
Q = 8192
INF = float("inf")


def _call(lib, g, **kw):
    a = dict(dict(q=P, qp=None, qn=None, x=P, x_bar=Q, x0=P, w=P, lo=-1.0, hi=2.0, tau=0.3, theta=0.5, flags=0, out=P, ws=P), **kw)
    return lib.tv_cp_primal_wls(ctypes.byref(g) if g is not None else None, a["q"], a["qp"], a["qn"], a["x"], a["x_bar"], a["x0"], a["w"],
                                a["lo"], a["hi"], a["tau"], a["theta"], a["flags"], a["out"], a["ws"], None)


def test_argument_errors_need_no_device():
    """an unknown flag bit, NULL g / arrays (w among them; x_bar in step mode only), x == x_bar, a NaN bound, a box without 0, tau that is
    <= 0 or not finite, theta outside [0, 1] or not finite in step mode, and a tv_geom of another interface version return TV_E_ARG, each
    with its own text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for flags in (2, 3, 4, -2, 1 << 30):
                assert _call(lib, g, flags=flags) == -1, flags
                assert b"flag" in lib.tv_last_error()
            for flags in (0, RESIDUAL):
                for name in ("q", "x", "x0", "w", "out", "ws") + (("x_bar",) if flags == 0 else ()):
                    assert _call(lib, g, flags=flags, **{name: None}) == -1, name
                    assert b"NULL" in lib.tv_last_error(), name
                assert _call(lib, g, flags=flags, x_bar=P) == -1
                assert b"x_bar" in lib.tv_last_error() and b"different" in lib.tv_last_error()
                for tau in (0.0, -0.25, float("nan"), INF, -INF):
                    assert _call(lib, g, flags=flags, tau=tau) == -1, tau
                    assert b"tau" in lib.tv_last_error() and b"theta" not in lib.tv_last_error()
                for bound in ("lo", "hi"):
                    assert _call(lib, g, flags=flags, **{bound: float("nan")}) == -1, bound
                    assert b"NaN" in lib.tv_last_error() and b"tau" not in lib.tv_last_error()
                for lo, hi in ((1e-300, 2.0), (1.0, 2.0), (-2.0, -1e-300), (-2.0, -1.0), (1.0, -1.0), (INF, INF), (-INF, -INF), (1.0, INF),
                               (-INF, -1.0)):
                    assert _call(lib, g, flags=flags, lo=lo, hi=hi) == -1, (lo, hi)
                    assert b"contain 0" in lib.tv_last_error() and b"pad" in lib.tv_last_error()
            for theta in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), INF):
                assert _call(lib, g, theta=theta) == -1, theta
                assert b"theta" in lib.tv_last_error()
    assert _call(lib, None) == -1
    assert b"tv_geom" in lib.tv_last_error()
    bad = _geom(nv)
    bad.abi_version = 4
    assert _call(lib, bad) == -1
    assert b"version" in lib.tv_last_error()


def test_boxes_that_contain_zero_pass_the_argument_checks():
    """(with every argument valid the halo check is the last one before the launch: on an interior slab without halo planes these calls return
    TV_E_HALO without following a pointer) -- infinite bounds, a degenerate box {0}, signed zeros"""
    from pytv import _native as nv
    lib = nv.lib()
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    for flags in (0, RESIDUAL):
        for lo, hi in ((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-1.0, 2.0), (0.0, 18.0), (-1e300, 1e-300)):
            assert _call(lib, g, flags=flags, lo=lo, hi=hi) == -2, (lo, hi)
            assert b"halo" in lib.tv_last_error()


def test_missing_gradient_halo_on_a_sharded_geometry_is_TV_E_HALO():
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
    assert _call(lib, g, w=None) == -1 and _call(lib, g, lo=0.5) == -1 and _call(lib, g, hi=-0.5) == -1 and _call(lib, g, hi=float("nan")) == -1


def test_solver_class_and_front_end_exist():
    import pytv
    cls = pytv.solvers.WeightedChambollePock
    assert issubclass(cls, pytv.solvers._ExtrapolatedCP) and issubclass(cls, pytv.solvers._FixedPointResiduals)
    assert "WeightedChambollePock" in pytv.solvers.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "weights", "lower", "upper", "scheme", "reg_z_over_reg", "reg_time", "mask_static",
                                         "factor_reg_static", "tau", "sigma", "slab", "pitch"]
    assert [init.parameters[k].default for k in list(init.parameters)[4:]] == [None, None, "hybrid", 1.0, 0.0, False, 0, None, None, None, "auto"]
    for name in ("step", "run", "run_steps", "result", "reset", "residuals", "initial_residual", "run_until"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_res", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert (cls.SLOTS, cls.F) == (pytv.solvers.ChambollePock.SLOTS, pytv.solvers.ChambollePock.F)
    doc = " ".join(cls.__doc__.split())
    # the model, the traffic, the shift, and what is not built
    for word in ("w_i = 0", "inpainting", "3 Nd + 6", "shift", "ACCELERATED", "Algorithm 1 only", "one-sweep", "hipGraph", "persistent", "x_init",
                 "per-voxel weights on the TV term"):
        assert word in doc, word
    assert "tv_cp_primal_wls" in cls.residuals.__doc__ and "tv_cp_primal_wls" in cls.run_until.__doc__
    # the residual plumbing is shared, not copied
    robust = pytv.solvers.RobustChambollePock
    for name in ("_residual_scalars", "_residual_dict", "initial_residual"):
        assert getattr(cls, name) is getattr(robust, name), name
    sig = inspect.signature(pytv.denoise_tv_weighted)
    assert pytv.denoise_tv_weighted is pytv.restoration.denoise_tv_weighted and "denoise_tv_weighted" in pytv.__all__
    assert "denoise_tv_weighted" in pytv.restoration.__all__
    assert list(sig.parameters) == ["image", "weights", "weight", "lower", "upper", "rel_res", "max_num_iter", "scheme", "tau", "check_every"]
    assert [sig.parameters[k].default for k in sig.parameters][2:] == [0.1, None, None, 1e-2, 400, "upwind", None, 10]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("scheme", "tau", "check_every"))
    # the other front-ends are as they were
    assert list(inspect.signature(pytv.denoise_tv_poisson).parameters) == ["image", "weight", "rel_res", "max_num_iter", "scheme", "tau",
                                                                           "check_every"]
