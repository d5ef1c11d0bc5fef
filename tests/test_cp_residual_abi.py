"""CPU-side checks of the optimality residual of ``ChambollePockOperator``: include/pytv4d.h declares tv_cp_dual_residual, the library exports
it, the ctypes table binds it; its argument and halo errors come back before anything touches the device; the solver has ``residuals``,
``run_until`` and the ``norm_A`` keyword; ``operator_norm_sq`` exists.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_header_declares_library_exports_binding_binds_tv_cp_dual_residual():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_cp_dual_residual\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_cp_dual_residual"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q", "double sigma_D",
                      "double lambda", "double* out", "void* ws", "void* stream"]
    assert code.index("tv_dual_gap") < m.start() < code.index("tv_cp_fused_supported")      # next to tv_dual_gap
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_cp_dual_residual")
    res, args = nv._SIGNATURES["tv_cp_dual_residual"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
    assert nv.lib().tv_cp_dual_residual.argtypes == args


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


def test_argument_errors_need_no_device():
    """NULL g / x / q / out, lambda and sigma_D that are <= 0 or NaN, and a tv_geom of another interface version return TV_E_ARG with a
    text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    P = 4096                                                      # any non-NULL value: argument checks come first
    ok = dict(x=P, xp=None, xn=None, q=P, sd=0.5, lam=5.0, out=P, ws=P)

    for dtype in (0, 1):
        g = _geom(nv, dtype=dtype)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.tv_cp_dual_residual(ctypes.byref(g), a["x"], a["xp"], a["xn"], a["q"], a["sd"], a["lam"], a["out"], a["ws"], None)

        for name in ("x", "q", "out"):
            assert call(**{name: None}) == -1, name
            assert b"NULL" in lib.tv_last_error(), name
        for lam in (0.0, -1.0, float("nan")):
            assert call(lam=lam) == -1
            assert b"lambda" in lib.tv_last_error()
        for sd in (0.0, -0.5, float("nan")):
            assert call(sd=sd) == -1
            assert b"sigma_D" in lib.tv_last_error()
    assert lib.tv_cp_dual_residual(None, P, None, None, P, 0.5, 5.0, P, P, None) == -1
    assert b"tv_geom" in lib.tv_last_error()
    bad = _geom(nv)
    bad.abi_version = 4
    assert lib.tv_cp_dual_residual(ctypes.byref(bad), P, None, None, P, 0.5, 5.0, P, P, None) == -1
    assert b"version" in lib.tv_last_error()


def test_missing_halo_on_a_sharded_geometry_is_TV_E_HALO():
    from pytv import _native as nv
    lib = nv.lib()
    P = 4096

    def call(g, xp, xn):
        return lib.tv_cp_dual_residual(ctypes.byref(g), P, xp, xn, P, 0.5, 5.0, P, P, None)

    for scheme in ("hybrid", "central"):                          # an interior slab: both image halo planes
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        assert call(g, None, P) == -2 and b"halo" in lib.tv_last_error()
        assert call(g, P, None) == -2 and b"halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # upwind looks forwards only, downwind backwards only
    assert call(up, P, None) == -2
    down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
    assert call(down, None, P) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert lib.tv_cp_dual_residual(ctypes.byref(g), P, None, None, P, 0.5, -1.0, P, P, None) == -1


def test_workspace_covers_the_two_sums():
    """the two per-block sums go through the existing partials layout: tv_workspace_bytes holds at least two slots of one partial per
    block of the scalar-lane launch (256 threads per block, one site each)"""
    from pytv import _native as nv
    lib = nv.lib()
    for shape in ((3, 2, 12, 20), (1, 1, 9, 13), (2, 1, 1024, 1024)):
        g = nv.new_geom()
        g.nz, g.m, g.ny, g.nx = shape
        g.nz_global, g.z0, g.scheme, g.dtype, g.reg_z_over_reg, g.reg_time = shape[0], 0, 3, 1, 1.0, 0.5
        nz, m, ny, nx = shape
        bx = 1
        while bx < nx and bx < 64:
            bx *= 2
        blocks = -(-nx // bx) * -(-ny // (256 // bx)) * m * nz
        assert lib.tv_workspace_bytes(ctypes.byref(g)) >= 2 * 8 * blocks


def test_solver_exposes_residuals_run_until_and_norm_A():
    import pytv
    cls = pytv.solvers.ChambollePockOperator
    assert callable(getattr(cls, "residuals")) and callable(getattr(cls, "run_until"))
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_res", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    doc = " ".join(cls.run_until.__doc__.split())
    assert "RELATIVE TO THE STARTING POINT" in doc and "x_init" in doc            # what rel_res means is documented
    init = inspect.signature(cls.__init__)
    assert init.parameters["norm_A"].default is None
    assert list(init.parameters)[-1] == "norm_A"                                   # appended: positional callers are not disturbed
    assert init.parameters["tau"].default is None


def test_operator_norm_sq_exists():
    import pytv
    sig = inspect.signature(pytv.solvers.operator_norm_sq)
    assert list(sig.parameters)[:5] == ["A", "AT", "like", "n_iter", "seed"]
    assert sig.parameters["n_iter"].default == 20 and sig.parameters["seed"].default == 0
    assert "operator_norm_sq" in pytv.solvers.__all__


def test_operator_norm_sq_on_the_cpu():
    """the helper is plain torch on whatever device ``like`` lives on: a diagonal operator with |A| = 3"""
    import torch
    import pytv
    like = torch.zeros((2, 2, 16, 16), dtype=torch.float64)
    a = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)[torch.arange(like.numel()) % 4].reshape(like.shape)
    calls = {"A": 0, "AT": 0}

    def A(v):
        calls["A"] += 1
        return a * v

    def AT(v):
        calls["AT"] += 1
        return a * v

    est = pytv.solvers.operator_norm_sq(A, AT, like)
    assert isinstance(est, float) and 9.0 <= est <= 9.0 * 1.06
    assert calls == {"A": 20, "AT": 20}
    assert pytv.solvers.operator_norm_sq(A, AT, like) == est                       # seeded
