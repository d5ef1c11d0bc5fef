"""CPU-side checks of the duality-gap certificate: include/pytv4d.h declares tv_dual_gap, the library exports it, the ctypes table binds it;
its argument and halo errors come back before anything touches the device; ChambollePock / ADMM have ``duality_gap`` and ``run_until``;
``denoise_tv_chambolle`` takes ``rel_gap``.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_header_declares_library_exports_binding_binds_tv_dual_gap():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_dual_gap\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_dual_gap"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q", "const void* q_prev",
                      "const void* q_next", "const void* x0", "double lambda", "double qscale", "double* out", "void* ws", "void* stream"]
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_dual_gap")
    res, args = nv._SIGNATURES["tv_dual_gap"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid"):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], 0
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


def test_argument_errors_need_no_device():
    """lambda <= 0, qscale == 0 and NULL x / q / x0 / out return TV_E_ARG with a text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    g = _geom(nv)
    P = 4096                                                      # any non-NULL value: argument checks come first
    ok = dict(x=P, xp=None, xn=None, q=P, qp=None, qn=None, x0=P, lam=5.0, qs=1.0, out=P, ws=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tv_dual_gap(ctypes.byref(g), a["x"], a["xp"], a["xn"], a["q"], a["qp"], a["qn"], a["x0"], a["lam"], a["qs"], a["out"], a["ws"], None)

    for name in ("x", "q", "x0", "out"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.tv_last_error(), name
    for lam in (0.0, -1.0, float("nan")):
        assert call(lam=lam) == -1
        assert b"lambda" in lib.tv_last_error()
    assert call(qs=0.0) == -1
    assert b"qscale" in lib.tv_last_error()
    bad = nv.new_geom()
    bad.abi_version = 4
    assert lib.tv_dual_gap(ctypes.byref(bad), P, None, None, P, None, None, P, 5.0, 1.0, P, P, None) == -1


def test_missing_halo_on_a_sharded_geometry_is_TV_E_HALO():
    from pytv import _native as nv
    lib = nv.lib()
    P = 4096
    g = _geom(nv, nz=3, nz_global=9, z0=3)                        # an interior slab: hybrid needs all four halo planes

    def call(xp, xn, qp, qn):
        return lib.tv_dual_gap(ctypes.byref(g), P, xp, xn, P, qp, qn, P, 5.0, 1.0, P, P, None)

    assert call(None, P, P, P) == -2 and b"halo" in lib.tv_last_error()
    assert call(P, None, P, P) == -2 and b"halo" in lib.tv_last_error()
    assert call(P, P, None, P) == -2 and b"gradient halo" in lib.tv_last_error()
    assert call(P, P, P, None) == -2 and b"gradient halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # upwind: x looks forwards, its adjoint backwards
    assert lib.tv_dual_gap(ctypes.byref(up), P, None, None, P, P, None, P, 5.0, 1.0, P, P, None) == -2
    assert lib.tv_dual_gap(ctypes.byref(up), P, None, P, P, None, None, P, 5.0, 1.0, P, P, None) == -2


def test_solvers_and_front_end_expose_the_certificate():
    import pytv
    for cls, limit, every in ((pytv.solvers.ChambollePock, "max_iter", 10), (pytv.solvers.ADMM, "max_outer", 5)):
        assert callable(getattr(cls, "duality_gap")) and callable(getattr(cls, "run_until"))
        sig = inspect.signature(cls.run_until)
        assert list(sig.parameters)[1:] == ["rel_gap", limit, "check_every"] and sig.parameters["check_every"].default == every
        assert "1e-6" in cls.run_until.__doc__ and "converged=False" in cls.run_until.__doc__       # the fp32 floor is documented
    assert not hasattr(pytv.solvers.SubgradientDescent, "duality_gap")                              # no dual variable, no certificate
    sig = inspect.signature(pytv.denoise_tv_chambolle)
    assert sig.parameters["rel_gap"].default is None and sig.parameters["rel_gap"].kind is inspect.Parameter.KEYWORD_ONLY
