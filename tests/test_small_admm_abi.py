"""CPU-side checks of the persistent ADMM entry point (round 7): the header declares tv_small_admm, the library exports it, the ctypes
table binds it, and pytv.solvers.ADMM has the ``persistent`` keyword with default False.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_header_declares_and_library_exports_tv_small_admm():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+tv_small_admm\s*\(([^;]*)\)\s*;", code, flags=re.M)
    assert m, "include/pytv4d.h does not declare tv_small_admm"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 20 and params[0] == "const tv_geom* g" and params[-1] == "void* stream"
    assert "const double* alpha" in params and "const double* beta" in params and "int64_t n_cheb" in params and "int64_t n_outer" in params
    assert "#define TV_ABI_VERSION 5" in src                     # an added function is compatible
    assert hasattr(ctypes.CDLL(nv.LIB_PATH), "tv_small_admm")
    res, args = nv._SIGNATURES["tv_small_admm"]
    assert res is ctypes.c_int and len(args) == len(params)


def test_argument_errors_need_no_device():
    """a refused geometry and NULL arrays return TV_E_ARG with a text before anything touches the device"""
    from pytv import _native as nv
    lib = nv.lib()
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = 3, 1, 8, 8, 6, 3          # a slab of a larger volume
    g.scheme, g.dtype = nv.SCHEMES["hybrid"], 0
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    al = (ctypes.c_double * 2)(0.5, 0.4)
    assert lib.tv_small_admm(ctypes.byref(g), *([None] * 8), 0.05, 1.0, al, al, 2, 1, None, 2, 1, None, None) == -1
    assert b"unsharded" in lib.tv_last_error()
    g.nz_global, g.z0 = 3, 0
    assert lib.tv_small_admm(ctypes.byref(g), *([None] * 8), 0.05, 1.0, al, al, 2, 1, None, 2, 1, None, None) == -1
    assert b"NULL" in lib.tv_last_error()


def test_admm_has_the_persistent_keyword_default_false():
    import pytv
    sig = inspect.signature(pytv.solvers.ADMM.__init__)
    assert "persistent" in sig.parameters and sig.parameters["persistent"].default is False
    assert pytv.solvers.ADMM.SMALL_MAX_CHEB == 32
