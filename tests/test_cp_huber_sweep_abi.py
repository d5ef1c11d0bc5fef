"""CPU-side checks of the one-sweep form of the Huber-TV Chambolle-Pock iteration: include/pytv4d.h declares tv_cp_huber_sweep with the agreed
parameter list and names tv_cp_accel_fixup as its fix-up, the library exports it, the ctypes table binds it, the interface version stays 5,
and every argument and halo error comes back -- each with its own text -- before a pointer is followed; ``HuberChambollePock`` has
``set_fused`` / ``fused`` and keeps its pinned signatures.  No GPU.  (The pattern of tests/test_cp_accel_sweep_abi.py.)"""
import ctypes
import inspect
import os
import re

from conftest import ROOT

SWEEP_PARAMS = ["const tv_geom* g", "const void* xbar_in", "const void* xbar_prev", "const void* xbar_next", "const void* q_in", "void* q_out",
                "const void* x0", "void* x", "void* xbar_out", "double sigma_D", "double lambda", "double alpha", "double tau", "double theta",
                "int32_t flags", "int64_t chunk_begin", "int64_t chunk_count", "double* hub", "double* fid", "void* ws", "void* stream"]


def _ctype_of(param):
    if param.startswith("double "):
        return ctypes.c_double
    if param.startswith("int32_t "):
        return ctypes.c_int32
    if param.startswith("int64_t "):
        return ctypes.c_int64
    return None                                                    # a pointer


def test_header_declares_library_exports_binding_binds_the_function():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "#define TV_ABI_VERSION 5" in src and nv.ABI_VERSION == 5 and nv.lib().tv_abi_version() == 5      # an added function is compatible
    handle = ctypes.CDLL(nv.LIB_PATH)
    name, want = "tv_cp_huber_sweep", SWEEP_PARAMS
    m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.M)
    assert m, "include/pytv4d.h does not declare " + name
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == want
    assert hasattr(handle, name)
    res, args = nv._SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(want)
    for a, p in zip(args, want):
        scalar = _ctype_of(p)
        assert (a is scalar) if scalar is not None else (a not in (ctypes.c_double, ctypes.c_int32, ctypes.c_int64)), (name, p)
    assert getattr(nv.lib(), name).argtypes == args
    # no fix-up symbol of its own: the header comment in front of the declaration sends the caller to tv_cp_accel_fixup, same tau and theta
    assert not hasattr(handle, "tv_cp_huber_fixup") and "tv_cp_huber_fixup" not in src
    comment = " ".join(src[:src.index("int tv_cp_huber_sweep(")].rsplit("/*", 1)[1].split())
    assert "tv_cp_accel_fixup" in comment and "same tau and theta" in comment


def _geom(nv, nx=64, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, nx, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


# any non-NULL, 16-byte aligned, pairwise different values: the checks come before the pointers are followed
XB_IN, XB_OUT, X, X0, Q_IN, Q_OUT, SC, WS, HALO = (4096 * k for k in range(1, 10))


def _sweep(lib, g, **kw):
    a = dict(dict(xbar_in=XB_IN, xp=None, xn=None, q_in=Q_IN, q_out=Q_OUT, x0=X0, x=X, xbar_out=XB_OUT, sigma=0.4, lam=5.0, alpha=2.0, tau=0.3,
                  theta=0.5, flags=0, cb=0, cc=-1, hub=SC, fid=SC + 64, ws=WS), **kw)
    return lib.tv_cp_huber_sweep(ctypes.byref(g) if g is not None else None, a["xbar_in"], a["xp"], a["xn"], a["q_in"], a["q_out"], a["x0"], a["x"],
                                 a["xbar_out"], a["sigma"], a["lam"], a["alpha"], a["tau"], a["theta"], a["flags"], a["cb"], a["cc"], a["hub"],
                                 a["fid"], a["ws"], None)


def test_argument_errors_need_no_device():
    from pytv import _native as nv
    lib = nv.lib()
    err = lib.tv_last_error
    for dtype in (0, 1):
        for scheme in ("hybrid", "central", "upwind", "downwind"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            assert lib.tv_cp_fused_supported(ctypes.byref(g)) == 1
            # ---- every case tv_cp_accel_sweep refuses
            for name in ("xbar_in", "q_in", "q_out", "x0", "x", "xbar_out", "hub", "fid", "ws"):
                assert _sweep(lib, g, **{name: None}) == -1, name
                assert b"NULL" in err(), name
            assert _sweep(lib, g, xbar_out=XB_IN) == -1
            assert b"xbar_in" in err() and b"xbar_out" in err() and b"different" in err()
            for other in (XB_IN, XB_OUT, X0):
                assert _sweep(lib, g, x=other) == -1
                assert b"alias" in err() and b"x0" in err()
            for lam in (0.0, -1.0, float("nan")):
                assert _sweep(lib, g, lam=lam) == -1
                assert b"lambda" in err()
            for tau in (0.0, -0.25, float("nan"), float("inf"), float("-inf")):
                assert _sweep(lib, g, tau=tau) == -1, tau
                assert b"tau" in err() and b"theta" not in err()
            for theta in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf")):
                assert _sweep(lib, g, theta=theta) == -1, theta
                assert b"theta" in err()
            for theta in (0.0, 1.0):                                              # the ends of [0, 1] pass (on to the range check, which stops the call)
                assert _sweep(lib, g, theta=theta, cb=7, cc=1) == -1 and b"chunk range" in err()
            for flags in (4, 8, -1):
                assert _sweep(lib, g, flags=flags) == -1
                assert b"tv_cp_huber_sweep: unknown flag" in err()
            assert _sweep(lib, g, flags=2) == -1
            assert b"TV_CP_FID_BOTH" in err() and b"TV_CP_FID_OF_INPUT" in err()
            for name in ("xbar_in", "q_in", "q_out", "x0", "x", "xbar_out"):
                assert _sweep(lib, g, **{name: dict(xbar_in=XB_IN, q_in=Q_IN, q_out=Q_OUT, x0=X0, x=X, xbar_out=XB_OUT)[name] + 8}) == -1, name
                assert b"aligned" in err(), name
            # ---- its own: alpha finite and > 0
            for alpha in (0.0, -2.0, float("nan"), float("inf"), float("-inf")):
                assert _sweep(lib, g, alpha=alpha) == -1, alpha
                assert b"alpha" in err() and b"tau" not in err() and b"lambda" not in err()
            for alpha in (1e-300, 1e300):                                         # any finite alpha > 0 passes (on to the range check)
                assert _sweep(lib, g, alpha=alpha, cb=7, cc=1) == -1 and b"chunk range" in err()
            assert _sweep(lib, g, cb=7, cc=1) == -1 and b"chunk range" in err()    # valid arguments reach the range check (and stop there)
            # ---- a geometry the one-sweep path refuses (nx < 64)
            small = _geom(nv, nx=8, dtype=dtype, scheme=scheme)
            assert lib.tv_cp_fused_supported(ctypes.byref(small)) == 0
            assert _sweep(lib, small) == -1 and b"not supported by the one-sweep path" in err()
            assert _sweep(lib, small, tau=-1.0) == -1 and b"tau" in err()           # the scalar checks come first
            assert _sweep(lib, small, alpha=0.0) == -1 and b"alpha" in err()
    assert _sweep(lib, None) == -1 and b"tv_geom" in err()
    bad = _geom(nv)
    bad.abi_version = 4
    assert _sweep(lib, bad) == -1 and b"version" in err()


def test_accel_sweep_keeps_its_messages():
    """the two entry points share one body: the accelerated sweep still names itself in its flag errors and takes no alpha"""
    from pytv import _native as nv
    lib = nv.lib()
    g = _geom(nv)
    r = lib.tv_cp_accel_sweep(ctypes.byref(g), XB_IN, None, None, Q_IN, Q_OUT, X0, X, XB_OUT, 0.4, 5.0, 0.3, 0.5, 8, 0, -1, SC, SC + 64, WS, None)
    assert r == -1 and b"tv_cp_accel_sweep: unknown flag" in lib.tv_last_error()
    r = lib.tv_cp_accel_sweep(ctypes.byref(g), XB_IN, None, None, Q_IN, Q_OUT, X0, X, XB_OUT, 0.4, 5.0, 0.3, 0.5, 0, 7, 1, SC, SC + 64, WS, None)
    assert r == -1 and b"chunk range" in lib.tv_last_error()


def test_missing_halo_plane_on_a_sharded_geometry_is_TV_E_HALO():
    """an interior slab: the sweep needs the planes of x_bar its differences read"""
    from pytv import _native as nv
    lib = nv.lib()
    for scheme in ("hybrid", "central"):
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        assert _sweep(lib, g, xp=None, xn=HALO) == -2 and b"halo" in lib.tv_last_error()
        assert _sweep(lib, g, xp=HALO, xn=None) == -2 and b"halo" in lib.tv_last_error()
    up = _geom(nv, nz=3, nz_global=9, z0=3, scheme="upwind")       # forward differences read x(z+1)
    assert _sweep(lib, up, xp=HALO, xn=None) == -2
    down = _geom(nv, nz=3, nz_global=9, z0=3, scheme="downwind")
    assert _sweep(lib, down, xp=None, xn=HALO) == -2
    g = _geom(nv, nz=3, nz_global=9, z0=3)                        # the argument checks come before the halo check
    assert _sweep(lib, g, tau=-1.0) == -1 and _sweep(lib, g, theta=1.5) == -1 and _sweep(lib, g, x=X0) == -1 and _sweep(lib, g, alpha=0.0) == -1


def test_solver_has_set_fused_and_keeps_its_pinned_signatures():
    import pytv
    cls = pytv.solvers.HuberChambollePock
    assert callable(cls.set_fused) and list(inspect.signature(cls.set_fused).parameters) == ["self", "fused"]
    assert isinstance(cls.fused, property) and cls.fused.fset is None                    # read-only
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ["x0", "regularization", "alpha", "scheme", "reg_z_over_reg", "reg_time",
                                                                    "mask_static", "factor_reg_static", "gamma", "slab", "pitch"]
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert list(inspect.signature(cls.run_until).parameters)[1:] == ["rel_gap", "max_iter", "check_every"]
    doc = " ".join(cls.__doc__.split())
    assert "tv_cp_huber_sweep" in doc and "tv_cp_accel_fixup" in doc and "a one-sweep / fix-up form of this iteration" not in doc
