"""CPU-side checks of the channel-coupled (vectorial) TV regulariser (one norm per spatial site over all frames and channels): include/pytv4d.h
declares tv_cp_dual_vtv and tv_dual_gap_vtv, the library exports them, the ctypes table binds them, and every argument and halo error comes back
before anything touches the device, each with a text that starts with the offending argument's name; the solver class and the front-end exist
with the documented signatures; tv_cp_dual, tv_dual_gap and the interface version are as they were.  No GPU."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

DUAL = ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "void* q", "double sigma_D",
        "double lambda", "double* vtv", "void* ws", "void* stream"]
GAP = ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q", "const void* q_prev",
       "const void* q_next", "const void* x0", "double lambda", "double* out", "void* ws", "void* stream"]


def _declared(code, name):
    m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.M)
    assert m, "include/pytv4d.h does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_library_exports_binding_binds_both_entry_points():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = ctypes.CDLL(nv.LIB_PATH)
    for name, want in (("tv_cp_dual_vtv", DUAL), ("tv_dual_gap_vtv", GAP)):
        params = _declared(code, name)
        assert params == want
        assert hasattr(so, name)
        res, args = nv._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params)
        assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
        assert getattr(nv.lib(), name).argtypes == args
    assert "#define TV_ABI_VERSION 5" in src and nv.lib().tv_abi_version() == 5          # added functions are compatible
    # the plain-TV dual step and gap were not extended
    assert _declared(code, "tv_cp_dual") == ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "void* q",
                                             "double sigma_D", "double lambda", "double* tv", "void* ws", "void* stream"]
    assert _declared(code, "tv_dual_gap") == ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q",
                                              "const void* q_prev", "const void* q_next", "const void* x0", "double lambda", "double qscale",
                                              "double* out", "void* ws", "void* stream"]
    assert len(nv._SIGNATURES["tv_cp_dual"][1]) == 10 and len(nv._SIGNATURES["tv_dual_gap"][1]) == 13
    # the model, the one-factor rule, the words per voxel of each form and what is exact are stated where the caller reads them
    comment = " ".join(src[src.index("CHANNEL-COUPLED"):src.index("int tv_cp_dual_vtv")].split())
    for word in ("|D x|_{F,s}", "ONE FACTOR PER SITE", "register form", "generic form", "2 Nd + 1 words", "3 Nd + 2 words", "bit for bit",
                 "never NaN or Inf", "TV_VTV_FORM", "no plane-marching form"):
        assert word in comment, word
    comment = " ".join(src[src.index("int tv_cp_dual_vtv"):src.index("int tv_dual_gap_vtv")].split())
    for word in ("EXACT", "Cauchy-Schwarz", "never as P - Dual", "not clamped", "REDUCE-ONLY"):
        assert word in comment, word


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0, m=3):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, m, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed


def _dual(lib, g, **kw):
    a = dict(dict(x=P, xp=None, xn=None, q=P, sigma=0.3, lam=5.0, out=P, ws=P), **kw)
    return lib.tv_cp_dual_vtv(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["sigma"], a["lam"],
                              a["out"], a["ws"], None)


def _gap(lib, g, **kw):
    a = dict(dict(x=P, xp=None, xn=None, q=P, qp=None, qn=None, x0=P, lam=5.0, out=P, ws=P), **kw)
    return lib.tv_dual_gap_vtv(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["qp"], a["qn"], a["x0"],
                               a["lam"], a["out"], a["ws"], None)


BAD = (0.0, -0.25, float("nan"), float("inf"), float("-inf"))
C_NAME = {"x": b"x ", "q": b"q ", "x0": b"x0 ", "ws": b"ws "}


def test_argument_errors_need_no_device():
    """NULL g / arrays, lambda or sigma_D that is not finite and > 0 and a tv_geom of another interface version return TV_E_ARG,
    each with its own text that starts with the offending name; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central", "upwind"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for call, arrays, scalars, out_name in ((_dual, ("x", "q", "out", "ws"), ("lam", "sigma"), b"vtv "),
                                                    (_gap, ("x", "q", "x0", "out", "ws"), ("lam",), b"out ")):
                texts = set()
                for name in arrays:
                    assert call(lib, g, **{name: None}) == -1, name
                    err = lib.tv_last_error()
                    assert b"NULL" in err and err.startswith(out_name if name == "out" else C_NAME[name]), (name, err)
                    texts.add(err)
                assert len(texts) == len(arrays)
                for name in scalars:
                    word = {"lam": b"lambda", "sigma": b"sigma_D"}[name]
                    for v in BAD:
                        assert call(lib, g, **{name: v}) == -1, (name, v)
                        err = lib.tv_last_error()
                        assert err.startswith(word), (name, v, err)
                assert call(lib, None) == -1
                assert b"tv_geom" in lib.tv_last_error()
                bad = _geom(nv, dtype=dtype, scheme=scheme)
                bad.abi_version = 4
                assert call(lib, bad) == -1
                assert b"version" in lib.tv_last_error()


def test_missing_halo_planes_on_a_sharded_geometry_are_refused():
    """a missing halo plane is refused with TV_E_HALO and a text that starts with the missing argument's name; with every argument valid the
    halo check is the last one before the launch: these calls return without following a pointer."""
    from pytv import _native as nv
    lib = nv.lib()
    for scheme in ("hybrid", "central"):                          # an interior slab: both halo planes of x, both of q
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        for call in (_dual, _gap):
            assert call(lib, g, xp=None, xn=P) == -2 and b"halo" in lib.tv_last_error() and lib.tv_last_error().startswith(b"x_prev")
            assert call(lib, g, xp=P, xn=None) == -2 and b"halo" in lib.tv_last_error() and lib.tv_last_error().startswith(b"x_next")
        assert _gap(lib, g, xp=P, xn=P, qp=None, qn=P) == -2 and lib.tv_last_error().startswith(b"q_prev") and b"halo" in lib.tv_last_error()
        assert _gap(lib, g, xp=P, xn=P, qp=P, qn=None) == -2 and lib.tv_last_error().startswith(b"q_next") and b"halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # a forward difference reads the next slab, its adjoint the previous one
    assert _dual(lib, up, xp=P, xn=None) == -2 and _gap(lib, up, xp=None, xn=P, qp=None, qn=None) == -2
    down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
    assert _dual(lib, down, xp=None, xn=P) == -2 and _gap(lib, down, xp=P, xn=None, qp=None, qn=None) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert _dual(lib, g, sigma=-1.0) == -1 and _dual(lib, g, lam=float("nan")) == -1 and _dual(lib, g, q=None) == -1
    assert _gap(lib, g, lam=0.0) == -1 and _gap(lib, g, x0=None) == -1


def test_solver_class_and_front_end_exist():
    import pytv
    S = pytv.solvers
    cls = S.VectorialTVChambollePock
    assert issubclass(cls, S._ExtrapolatedCP) and issubclass(cls, S._GapStopping) and "VectorialTVChambollePock" in S.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "scheme", "reg_z_over_reg", "reg_time", "mask_static", "factor_reg_static",
                                         "tau0", "sigma0", "gamma", "slab", "pitch"]
    assert [init.parameters[k].default for k in list(init.parameters)[3:]] == ["hybrid", 1.0, 0.0, False, 0, None, None, 1.0, None, "auto"]
    assert init == inspect.signature(S.AcceleratedChambollePock.__init__)
    for name in ("step", "run", "run_steps", "result", "reset", "duality_gap", "run_until", "set_fused"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_gap", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert (cls.SLOTS, cls.F) == (S.ChambollePock.SLOTS, S.ChambollePock.F)
    # the loop, the schedule and the exchanges are the bases'
    for name in ("run_steps", "reset", "_run", "_dual_half", "_alloc_state", "_primal_kernel"):
        assert getattr(cls, name) is getattr(S._ExtrapolatedCP, name), name
    for name in ("_steps", "step", "run"):
        assert getattr(cls, name) is getattr(S.AcceleratedChambollePock, name), name
    assert cls._gap_certificate is S._SlabProblem._gap_certificate and cls._run_until_gap is S._SlabProblem._run_until_gap
    # ... and the bases keep their own kernels
    assert cls._dual_kernel is not S._ExtrapolatedCP._dual_kernel and cls._gap_kernel is not S._SlabProblem._gap_kernel
    assert S.AcceleratedChambollePock._dual_kernel is S._ExtrapolatedCP._dual_kernel
    assert S.AcceleratedChambollePock._gap_kernel is S._SlabProblem._gap_kernel
    assert S.AdaptiveTVChambollePock._dual_kernel is not cls._dual_kernel
    assert "tv_cp_dual_vtv" in inspect.getsource(cls._dual_kernel) and "tv_dual_gap_vtv" in inspect.getsource(cls._gap_kernel)
    doc = " ".join(cls.__doc__.split())
    for word in ("sum_s |D x|_{F,s}", "multi-energy", "colour", "ONE factor per site", "2 Nd + 1 words", "3 Nd + 2", "Algorithm 2", "bit for bit",
                 "one-sweep", "persistent", "hipGraph", "plane-marching", "per-voxel weight", "Huber", "ADMM", "SubgradientDescent"):
        assert word in doc, word
    for fn in (cls.duality_gap, cls.run_until):
        assert "tv_dual_gap_vtv" in fn.__doc__ and "fp32 FLOOR" in fn.__doc__
    assert "VectorialTVChambollePock" in " ".join(S.AcceleratedChambollePock.__doc__.split())
    # the one-sweep path is refused without a device: set_fused(True) raises before it looks at anything, and names the class
    obj = object.__new__(cls)
    with pytest.raises(ValueError, match="VectorialTVChambollePock.*one-sweep"):
        obj.set_fused(True)
    obj.set_fused(None)
    assert obj.fused is False
    obj.set_fused(False)
    assert obj.fused is False
    # regularization is checked before x0 is looked at
    for reg in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="regularization"):
            cls(None, reg)
    sig = inspect.signature(pytv.denoise_tv_vectorial)
    assert pytv.denoise_tv_vectorial is pytv.restoration.denoise_tv_vectorial and "denoise_tv_vectorial" in pytv.__all__
    assert "denoise_tv_vectorial" in pytv.restoration.__all__
    assert list(sig.parameters) == ["image", "weight", "channel_axis", "rel_gap", "max_num_iter", "scheme", "check_every"]
    assert [sig.parameters[k].default for k in sig.parameters][1:] == [0.1, 0, 1e-4, 200, "upwind", 10]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("scheme", "check_every"))
    # ... with the defaults and conventions of denoise_tv_adaptive
    other = inspect.signature(pytv.denoise_tv_adaptive)
    for k in ("weight", "rel_gap", "max_num_iter", "scheme", "check_every"):
        assert (sig.parameters[k].default, sig.parameters[k].kind) == (other.parameters[k].default, other.parameters[k].kind), k
    # the other front-ends are as they were
    assert list(other.parameters) == ["image", "weight", "reg_weights", "rel_gap", "max_num_iter", "scheme", "check_every"]


def test_option_that_forces_a_form_is_known():
    from pytv import _native as nv
    unset = -2 ** 31
    assert nv.get_option("TV_VTV_FORM", unset) in (unset, 0, 2)
    before = nv.get_option("TV_VTV_FORM", unset)
    nv.set_option("TV_VTV_FORM", 2)
    assert nv.get_option("TV_VTV_FORM", 0) == 2
    nv.set_option("TV_VTV_FORM", None if before == unset else before)
    assert nv.get_option("TV_VTV_FORM", unset) == before
