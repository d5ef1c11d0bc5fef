"""CPU-side checks of the Huber-TV regulariser: include/pytv4d.h declares tv_cp_dual_huber and tv_dual_gap_huber, the library exports them, the
ctypes table binds them, and every argument and halo error comes back before anything touches the device; ``cp_linear_steps`` against its
closed form; the solver class and the front-end exist with the documented signatures; tv_cp_dual and the interface version are as they were.
No GPU."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import ROOT

DUAL = ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "void* q", "double sigma_D", "double lambda",
        "double alpha", "double* hubout", "void* ws", "void* stream"]
GAP = ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q", "const void* q_prev",
       "const void* q_next", "const void* x0", "double lambda", "double alpha", "double* out", "void* ws", "void* stream"]


def _declared(code, name):
    m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.M)
    assert m, "include/pytv4d.h does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_library_exports_binding_binds_both_entry_points():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = ctypes.CDLL(nv.LIB_PATH)
    for name, want in (("tv_cp_dual_huber", DUAL), ("tv_dual_gap_huber", GAP)):
        params = _declared(code, name)
        assert params == want
        assert hasattr(so, name)
        res, args = nv._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params)
        assert [a is ctypes.c_double for a in args] == [p.startswith("double ") for p in params]
        assert getattr(nv.lib(), name).argtypes == args
    assert "#define TV_ABI_VERSION 5" in src and nv.lib().tv_abi_version() == 5          # added functions are compatible
    # the plain-TV dual step was not extended
    assert _declared(code, "tv_cp_dual") == ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "void* q",
                                             "double sigma_D", "double lambda", "double* tv", "void* ws", "void* stream"]
    assert len(nv._SIGNATURES["tv_cp_dual"][1]) == 10


def _geom(nv, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, 8, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


P = 4096                                                          # any non-NULL value: the checks come before the pointers are followed


def _dual(lib, g, **kw):
    a = dict(dict(x=P, xp=None, xn=None, q=P, sigma=0.3, lam=5.0, alpha=0.5, out=P, ws=P), **kw)
    return lib.tv_cp_dual_huber(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["sigma"], a["lam"], a["alpha"],
                                a["out"], a["ws"], None)


def _gap(lib, g, **kw):
    a = dict(dict(x=P, xp=None, xn=None, q=P, qp=None, qn=None, x0=P, lam=5.0, alpha=0.5, out=P, ws=P), **kw)
    return lib.tv_dual_gap_huber(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["qp"], a["qn"], a["x0"],
                                 a["lam"], a["alpha"], a["out"], a["ws"], None)


BAD = (0.0, -0.25, float("nan"), float("inf"), float("-inf"))


def test_argument_errors_need_no_device():
    """NULL g / arrays, lambda, alpha or sigma_D that is not finite and > 0 (alpha = 0 included: that model is tv_cp_dual) and a tv_geom of
    another interface version return TV_E_ARG, each with its own text; the pointers are never followed"""
    from pytv import _native as nv
    lib = nv.lib()
    for dtype in (0, 1):
        for scheme in ("hybrid", "central", "upwind"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            for call, arrays, scalars in ((_dual, ("x", "q", "out", "ws"), ("lam", "alpha", "sigma")),
                                          (_gap, ("x", "q", "x0", "out", "ws"), ("lam", "alpha"))):
                for name in arrays:
                    assert call(lib, g, **{name: None}) == -1, name
                    assert b"NULL" in lib.tv_last_error(), name
                for name in scalars:
                    word = {"lam": b"lambda", "alpha": b"alpha", "sigma": b"sigma_D"}[name]
                    others = [w for w in (b"lambda", b"alpha", b"sigma_D") if w != word]
                    for v in BAD:
                        assert call(lib, g, **{name: v}) == -1, (name, v)
                        err = lib.tv_last_error()
                        assert err.startswith(word) and not any(err.startswith(w) for w in others), (name, v, err)
                assert call(lib, None) == -1
                assert b"tv_geom" in lib.tv_last_error()
                bad = _geom(nv, dtype=dtype, scheme=scheme)
                bad.abi_version = 4
                assert call(lib, bad) == -1
                assert b"version" in lib.tv_last_error()
    assert _dual(lib, g, alpha=0.0) == -1
    assert b"tv_cp_dual" in lib.tv_last_error()                     # the refusal says where alpha = 0 lives


def test_missing_halo_planes_on_a_sharded_geometry_are_refused():
    """a missing halo plane is refused with a text of its own and the code every entry point here gives it, TV_E_HALO (tv_cp_dual's rule,
    include/pytv4d.h); with every argument valid the halo check is the last one before the launch: these calls return without following a
    pointer"""
    from pytv import _native as nv
    lib = nv.lib()
    for scheme in ("hybrid", "central"):                          # an interior slab: both halo planes of x, both of q
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        for call in (_dual, _gap):
            assert call(lib, g, xp=None, xn=P) == -2 and b"halo" in lib.tv_last_error() and b"previous" in lib.tv_last_error()
            assert call(lib, g, xp=P, xn=None) == -2 and b"halo" in lib.tv_last_error() and b"next" in lib.tv_last_error()
        assert _gap(lib, g, xp=P, xn=P, qp=None, qn=P) == -2 and b"gradient halo" in lib.tv_last_error()
        assert _gap(lib, g, xp=P, xn=P, qp=P, qn=None) == -2 and b"gradient halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # a forward difference reads the next slab, its adjoint the previous one
    assert _dual(lib, up, xp=P, xn=None) == -2 and _gap(lib, up, xp=None, xn=P, qp=None, qn=None) == -2
    down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
    assert _dual(lib, down, xp=None, xn=P) == -2 and _gap(lib, down, xp=P, xn=None, qp=None, qn=None) == -2
    # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3)
    assert _dual(lib, g, alpha=0.0) == -1 and _dual(lib, g, sigma=-1.0) == -1 and _dual(lib, g, lam=float("nan")) == -1 and _dual(lib, g, q=None) == -1
    assert _gap(lib, g, alpha=float("inf")) == -1 and _gap(lib, g, lam=0.0) == -1 and _gap(lib, g, x0=None) == -1


def test_cp_linear_steps():
    from pytv.solvers import cp_linear_steps
    for L2, gamma, delta in ((8.0, 1.0, 0.05), (8.0, 1.0, 0.2), (2.95, 1.0, 0.05), (11.8, 0.5, 0.2), (12.0, 0.3, 1e-3), (1e-2, 1.0, 7.0)):
        tau, sigma, theta, mu = cp_linear_steps(L2, gamma, delta)
        want_mu = 2.0 * math.sqrt(gamma * delta) / math.sqrt(L2)
        assert all(isinstance(v, float) for v in (tau, sigma, theta, mu))
        assert abs(mu - want_mu) <= 4e-16 * want_mu
        assert abs(tau - want_mu / (2.0 * gamma)) <= 4e-16 * tau and abs(sigma - want_mu / (2.0 * delta)) <= 1e-15 * sigma
        assert abs(theta - 1.0 / (1.0 + want_mu)) <= 4e-16 and 0.0 < theta < 1.0
        assert abs(tau * sigma * L2 - 1.0) <= 1e-15
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        for args in ((bad, 1.0, 0.1), (8.0, bad, 0.1), (8.0, 1.0, bad)):
            with pytest.raises(ValueError, match="cp_linear_steps"):
                cp_linear_steps(*args)


def test_solver_class_and_front_end_exist():
    import pytv
    cls = pytv.solvers.HuberChambollePock
    assert issubclass(cls, pytv.solvers._ExtrapolatedCP) and "HuberChambollePock" in pytv.solvers.__all__ and "cp_linear_steps" in pytv.solvers.__all__
    init = inspect.signature(cls.__init__)
    assert list(init.parameters)[1:] == ["x0", "regularization", "alpha", "scheme", "reg_z_over_reg", "reg_time", "mask_static", "factor_reg_static",
                                         "gamma", "slab", "pitch"]
    assert [init.parameters[k].default for k in list(init.parameters)[4:]] == ["hybrid", 1.0, 0.0, False, 0, 1.0, None, "auto"]
    assert init.parameters["alpha"].default is inspect.Parameter.empty
    for name in ("step", "run", "run_steps", "result", "reset", "duality_gap", "run_until"):
        assert callable(getattr(cls, name)), name
    sig = inspect.signature(cls.run_until)
    assert list(sig.parameters)[1:] == ["rel_gap", "max_iter", "check_every"] and sig.parameters["check_every"].default == 10
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert (cls.SLOTS, cls.F) == (pytv.solvers.ChambollePock.SLOTS, pytv.solvers.ChambollePock.F)
    # run / run_steps / reset and the dual half's exchanges come from the base
    for name in ("run_steps", "reset", "_run", "_dual_half", "_alloc_state"):
        assert getattr(cls, name) is getattr(pytv.solvers._ExtrapolatedCP, name), name
    assert cls._gap_certificate is pytv.solvers._SlabProblem._gap_certificate and cls._run_until_gap is pytv.solvers._SlabProblem._run_until_gap
    doc = " ".join(cls.__doc__.split())
    for word in ("gradient magnitude", "grey levels per weighted difference", "Algorithm 3", "AcceleratedChambollePock", "mu -> 0",
                 "one-sweep", "persistent", "hipGraph", "placement tuner", "L1 / Huber / KL"):          # the model, alpha, and what is not built
        assert word in doc, word
    assert "tv_dual_gap_huber" in cls.duality_gap.__doc__ and "tv_dual_gap_huber" in cls.run_until.__doc__
    for sibling in ("AcceleratedChambollePock", "RobustChambollePock", "PoissonChambollePock"):
        assert "HuberChambollePock" in " ".join(getattr(pytv.solvers, sibling).__doc__.split()), sibling
    sig = inspect.signature(pytv.denoise_tv_huber)
    assert pytv.denoise_tv_huber is pytv.restoration.denoise_tv_huber and "denoise_tv_huber" in pytv.__all__
    assert "denoise_tv_huber" in pytv.restoration.__all__
    assert list(sig.parameters) == ["image", "weight", "alpha", "rel_gap", "max_num_iter", "scheme", "check_every"]
    assert [sig.parameters[k].default for k in sig.parameters][1:] == [0.1, 1.0, 1e-4, 200, "upwind", 10]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("scheme", "check_every"))
    # the other front-ends are as they were
    assert list(inspect.signature(pytv.denoise_tv_poisson).parameters) == ["image", "weight", "rel_res", "max_num_iter", "scheme", "tau", "check_every"]
