"""CPU-side checks of the adaptive Huber-TV solver: include/pytv4d.h declares tv_cp_dual_hwtv, tv_dual_gap_hwtv and tv_cp_hwtv_sweep with the agreed
parameter lists, the library exports them, the ctypes table binds them, the interface version stays 5, argument and halo errors come back --
each naming its argument -- before a pointer is followed; ``AdaptiveHuberChambollePock`` and ``denoise_tv_adaptive_huber`` have the agreed
surface and the three kernel hooks name the right entry points.  No GPU.  (The pattern of tests/test_cp_huber_sweep_abi.py / test_cp_wtv_abi.py.)"""
import ctypes
import inspect
import os
import re

from conftest import ROOT

PARAMS = {
    "tv_cp_dual_hwtv": ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "void* q", "const void* gw",
                        "double sigma_D", "double lambda", "double alpha", "double* hwtv", "void* ws", "void* stream"],
    "tv_dual_gap_hwtv": ["const tv_geom* g", "const void* x", "const void* x_prev", "const void* x_next", "const void* q", "const void* q_prev",
                         "const void* q_next", "const void* x0", "const void* gw", "double lambda", "double alpha", "double* out", "void* ws",
                         "void* stream"],
    "tv_cp_hwtv_sweep": ["const tv_geom* g", "const void* xbar_in", "const void* xbar_prev", "const void* xbar_next", "const void* q_in",
                         "void* q_out", "const void* x0", "void* x", "void* xbar_out", "const void* gw", "double sigma_D", "double lambda",
                         "double alpha", "double tau", "double theta", "int32_t flags", "int64_t chunk_begin", "int64_t chunk_count",
                         "double* hwtv", "double* fid", "void* ws", "void* stream"],
}


def _ctype_of(param):
    if param.startswith("double "):
        return ctypes.c_double
    if param.startswith("int32_t "):
        return ctypes.c_int32
    if param.startswith("int64_t "):
        return ctypes.c_int64
    return None                                                    # a pointer


def test_header_declares_library_exports_binding_binds_the_three_functions():
    from pytv import _native as nv
    src = open(os.path.join(ROOT, "include", "pytv4d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "#define TV_ABI_VERSION 5" in src and nv.ABI_VERSION == 5 and nv.lib().tv_abi_version() == 5      # added functions are compatible
    handle = ctypes.CDLL(nv.LIB_PATH)
    for name, want in PARAMS.items():
        m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.M)
        assert m, "include/pytv4d.h does not declare " + name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == want, name
        assert hasattr(handle, name), name
        res, args = nv._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(want), name
        for a, p in zip(args, want):
            scalar = _ctype_of(p)
            assert (a is scalar) if scalar is not None else (a not in (ctypes.c_double, ctypes.c_int32, ctypes.c_int64)), (name, p)
        assert getattr(nv.lib(), name).argtypes == args
    # no fix-up symbol of its own: the comment in front of the sweep's declaration sends the caller to tv_cp_accel_fixup, same tau and theta
    assert not hasattr(handle, "tv_cp_hwtv_fixup") and "tv_cp_hwtv_fixup" not in src
    comment = " ".join(src[:src.index("int tv_cp_hwtv_sweep(")].rsplit("/*", 1)[1].split())
    assert "tv_cp_accel_fixup" in comment and "same tau and theta" in comment and "NO halo plane" in comment


def _geom(nv, nx=64, nz=3, nz_global=3, z0=0, scheme="hybrid", dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, 1, 8, nx, nz_global, z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time = 1.0, 0.0
    return g


# any non-NULL, 16-byte aligned, pairwise different values: the checks come before the pointers are followed
XB_IN, XB_OUT, X, X0, Q_IN, Q_OUT, SC, WS, HALO, GW = (4096 * k for k in range(1, 11))


def _dual(lib, g, **kw):
    a = dict(dict(x=X, xp=None, xn=None, q=Q_IN, gw=GW, sigma=0.4, lam=5.0, alpha=2.0, hwtv=SC, ws=WS), **kw)
    return lib.tv_cp_dual_hwtv(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["gw"], a["sigma"], a["lam"],
                               a["alpha"], a["hwtv"], a["ws"], None)


def _gap(lib, g, **kw):
    a = dict(dict(x=X, xp=None, xn=None, q=Q_IN, qp=None, qn=None, x0=X0, gw=GW, lam=5.0, alpha=2.0, out=SC, ws=WS), **kw)
    return lib.tv_dual_gap_hwtv(ctypes.byref(g) if g is not None else None, a["x"], a["xp"], a["xn"], a["q"], a["qp"], a["qn"], a["x0"], a["gw"],
                                a["lam"], a["alpha"], a["out"], a["ws"], None)


def _sweep(lib, g, **kw):
    a = dict(dict(xbar_in=XB_IN, xp=None, xn=None, q_in=Q_IN, q_out=Q_OUT, x0=X0, x=X, xbar_out=XB_OUT, gw=GW, sigma=0.4, lam=5.0, alpha=2.0,
                  tau=0.3, theta=0.5, flags=0, cb=0, cc=-1, hwtv=SC, fid=SC + 64, ws=WS), **kw)
    return lib.tv_cp_hwtv_sweep(ctypes.byref(g) if g is not None else None, a["xbar_in"], a["xp"], a["xn"], a["q_in"], a["q_out"], a["x0"], a["x"],
                                a["xbar_out"], a["gw"], a["sigma"], a["lam"], a["alpha"], a["tau"], a["theta"], a["flags"], a["cb"], a["cc"],
                                a["hwtv"], a["fid"], a["ws"], None)


BAD_POSITIVE = (0.0, -2.0, float("nan"), float("inf"), float("-inf"))


def test_one_site_entry_points_name_the_offending_argument():
    """as tv_cp_dual_wtv / tv_dual_gap_wtv name theirs ("<name> is NULL"), with tv_cp_dual_huber's alpha; a missing halo plane is TV_E_HALO with
    the argument's name in front"""
    from pytv import _native as nv
    lib = nv.lib()
    err = lib.tv_last_error
    for dtype in (0, 1):
        for scheme in ("hybrid", "central", "upwind", "downwind"):
            g = _geom(nv, nx=20, dtype=dtype, scheme=scheme)                      # any geometry: scalar rows too
            for name in ("x", "q", "gw", "hwtv", "ws"):
                assert _dual(lib, g, **{name: None}) == -1 and err() == (name + " is NULL").encode(), name
            for name in ("x", "q", "x0", "gw", "out", "ws"):
                assert _gap(lib, g, **{name: None}) == -1 and err() == (name + " is NULL").encode(), name
            for call in (_dual, _gap):
                for v in BAD_POSITIVE:
                    assert call(lib, g, alpha=v) == -1 and b"alpha" in err() and b"lambda" not in err(), (call.__name__, v)
                    assert call(lib, g, lam=v) == -1 and b"lambda" in err() and b"alpha" not in err(), (call.__name__, v)
            for v in BAD_POSITIVE:
                assert _dual(lib, g, sigma=v) == -1 and b"sigma_D" in err(), v
    assert _dual(lib, None) == -1 and b"tv_geom" in err()
    assert _gap(lib, None) == -1 and b"tv_geom" in err()
    bad = _geom(nv)
    bad.abi_version = 4
    assert _dual(lib, bad) == -1 and b"version" in err()
    assert _gap(lib, bad) == -1 and b"version" in err()
    # an interior slab without a halo plane its scheme reads
    for scheme, sides in (("hybrid", ("prev", "next")), ("central", ("prev", "next")), ("upwind", ("next",)), ("downwind", ("prev",))):
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        for side in sides:
            kw = dict(dict(xp=HALO, xn=HALO), **{"xp" if side == "prev" else "xn": None})
            assert _dual(lib, g, **kw) == -2 and err().startswith(b"x_%s: " % side.encode()) and b"halo" in err(), (scheme, side)
            assert _gap(lib, g, qp=HALO, qn=HALO, **kw) == -2 and err().startswith(b"x_%s: " % side.encode()), (scheme, side)
        assert _dual(lib, g, xp=HALO, xn=HALO, alpha=0.0) == -1                     # the argument checks come before the halo check
    g = _geom(nv, nz=3, nz_global=9, z0=3, scheme="hybrid")
    assert _gap(lib, g, xp=HALO, xn=HALO, qp=None, qn=HALO) == -2 and err().startswith(b"q_prev: ")
    assert _gap(lib, g, xp=HALO, xn=HALO, qp=HALO, qn=None) == -2 and err().startswith(b"q_next: ")


def test_sweep_argument_errors_need_no_device():
    from pytv import _native as nv
    lib = nv.lib()
    err = lib.tv_last_error
    for dtype in (0, 1):
        for scheme in ("hybrid", "central", "upwind", "downwind"):
            g = _geom(nv, dtype=dtype, scheme=scheme)
            assert lib.tv_cp_fused_supported(ctypes.byref(g)) == 1
            # ---- every case tv_cp_accel_sweep refuses
            for name in ("xbar_in", "q_in", "q_out", "x0", "x", "xbar_out", "hwtv", "fid", "ws"):
                assert _sweep(lib, g, **{name: None}) == -1 and b"NULL" in err(), name
            assert _sweep(lib, g, xbar_out=XB_IN) == -1 and b"different" in err()
            for other in (XB_IN, XB_OUT, X0):
                assert _sweep(lib, g, x=other) == -1 and b"alias" in err()
            for tau in (0.0, -0.25, float("nan"), float("inf")):
                assert _sweep(lib, g, tau=tau) == -1 and b"tau" in err() and b"theta" not in err(), tau
            for theta in (-1e-9, 1.0 + 1e-9, float("nan")):
                assert _sweep(lib, g, theta=theta) == -1 and b"theta" in err(), theta
            for flags in (4, 8, -1):
                assert _sweep(lib, g, flags=flags) == -1 and b"tv_cp_hwtv_sweep: unknown flag" in err()
            assert _sweep(lib, g, flags=2) == -1 and b"TV_CP_FID_BOTH" in err()
            for name in ("xbar_in", "q_in", "q_out", "x0", "x", "xbar_out", "gw"):
                off = dict(xbar_in=XB_IN, q_in=Q_IN, q_out=Q_OUT, x0=X0, x=X, xbar_out=XB_OUT, gw=GW)[name] + 8
                assert _sweep(lib, g, **{name: off}) == -1 and b"aligned" in err(), name
            # ---- its own: gw, and lambda / alpha / sigma_D finite and > 0
            assert _sweep(lib, g, gw=None) == -1 and err() == b"gw is NULL"
            for v in BAD_POSITIVE:
                assert _sweep(lib, g, alpha=v) == -1 and b"alpha" in err() and b"tau" not in err(), v
                assert _sweep(lib, g, lam=v) == -1 and b"lambda" in err(), v
                assert _sweep(lib, g, sigma=v) == -1 and b"sigma_D" in err(), v
            for alpha in (1e-300, 1e300):                                         # any finite alpha > 0 passes (on to the range check)
                assert _sweep(lib, g, alpha=alpha, cb=7, cc=1) == -1 and b"chunk range" in err()
            small = _geom(nv, nx=8, dtype=dtype, scheme=scheme)
            assert _sweep(lib, small) == -1 and b"not supported by the one-sweep path" in err()
    assert _sweep(lib, None) == -1 and b"tv_geom" in err()
    for scheme in ("hybrid", "central"):
        g = _geom(nv, nz=3, nz_global=9, z0=3, scheme=scheme)
        assert _sweep(lib, g, xp=None, xn=HALO) == -2 and b"halo" in err()
        assert _sweep(lib, g, xp=HALO, xn=None) == -2 and b"halo" in err()
    # the siblings that share the body keep their own messages and take no gw
    g = _geom(nv)
    r = lib.tv_cp_huber_sweep(ctypes.byref(g), XB_IN, None, None, Q_IN, Q_OUT, X0, X, XB_OUT, 0.4, 5.0, 2.0, 0.3, 0.5, 8, 0, -1, SC, SC + 64, WS, None)
    assert r == -1 and b"tv_cp_huber_sweep: unknown flag" in err()
    r = lib.tv_cp_accel_sweep(ctypes.byref(g), XB_IN, None, None, Q_IN, Q_OUT, X0, X, XB_OUT, 0.4, 5.0, 0.3, 0.5, 0, 7, 1, SC, SC + 64, WS, None)
    assert r == -1 and b"chunk range" in err()


HUBER_TAIL = ["scheme", "reg_z_over_reg", "reg_time", "mask_static", "factor_reg_static", "gamma", "slab", "pitch"]


def test_class_surface_front_end_and_exports():
    import pytv
    S = pytv.solvers
    cls, hub = S.AdaptiveHuberChambollePock, S.HuberChambollePock
    assert "AdaptiveHuberChambollePock" in S.__all__
    assert cls.__mro__[1:3] == (S._GapStopping, S._OneSweepCP) and issubclass(cls, S._ExtrapolatedCP)
    assert not issubclass(cls, (S.AcceleratedChambollePock, hub, S.AdaptiveTVChambollePock))
    sig, hsig = inspect.signature(cls.__init__).parameters, inspect.signature(hub.__init__).parameters
    assert list(sig)[1:] == ["x0", "regularization", "reg_weights", "alpha"] + HUBER_TAIL
    for name in HUBER_TAIL:                                        # the remaining keywords and their defaults are HuberChambollePock's
        assert sig[name].default == hsig[name].default and sig[name].kind == hsig[name].kind, name
    assert all(sig[n].default is inspect.Parameter.empty for n in ("x0", "regularization", "reg_weights", "alpha"))
    # the paths come from _OneSweepCP unchanged, the stopping rule from _GapStopping / _SlabProblem
    assert cls.set_fused is S._OneSweepCP.set_fused and "set_fused" not in vars(cls)
    assert isinstance(cls.fused, property) and cls.fused.fset is None and cls.fused.fget is S._OneSweepCP.fused.fget
    assert "_gap_certificate" not in vars(cls) and "_run_until_gap" not in vars(cls) and "_one_sweep" not in vars(cls)
    assert list(inspect.signature(cls.run).parameters)[1:] == ["n_iter", "record_loss"]
    assert list(inspect.signature(cls.run_until).parameters)[1:] == ["rel_gap", "max_iter", "check_every"]
    assert list(inspect.signature(cls.duality_gap).parameters) == ["self"]
    doc = " ".join(cls.__doc__.split())
    for word in ("tv_cp_dual_hwtv", "tv_cp_hwtv_sweep", "tv_cp_accel_fixup", "tv_dual_gap_hwtv", "2 Nd + 6", "3 Nd + 6", "g_max", "per-voxel alpha"):
        assert word in doc, word
    for sibling in ("HuberChambollePock", "AdaptiveTVChambollePock"):
        assert "AdaptiveHuberChambollePock" in " ".join(getattr(S, sibling).__doc__.split()), sibling
    # AdaptiveTVChambollePock keeps its refusal
    assert "set_fused" in vars(S.AdaptiveTVChambollePock)
    # the front-end
    f = pytv.denoise_tv_adaptive_huber
    assert f is pytv.restoration.denoise_tv_adaptive_huber
    assert "denoise_tv_adaptive_huber" in pytv.__all__ and "denoise_tv_adaptive_huber" in pytv.restoration.__all__
    p = inspect.signature(f).parameters
    assert list(p) == ["image", "weight", "reg_weights", "alpha", "rel_gap", "max_num_iter", "scheme", "check_every"]
    assert [p[n].default for n in list(p)[1:]] == [0.1, None, 1.0, 1e-4, 200, "upwind", 10]
    assert p["scheme"].kind is inspect.Parameter.KEYWORD_ONLY and p["check_every"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["max_num_iter"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


class _Recorder:
    """stands in for the library: records the name of every entry point called and returns success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_kernel_hooks_name_the_right_entry_points():
    """the three hooks on an object that has only what they read: each makes ONE library call, of the agreed name, with g and alpha in the
    agreed positions"""
    import pytv
    from pytv import _native as nv
    cls = pytv.solvers.AdaptiveHuberChambollePock
    me = object.__new__(cls)
    rec = _Recorder()
    me.lib, me.reg, me.alpha = rec, 5.0, 2.0
    me.geo = type("G", (), {"ref": "GEO"})()
    for k in ("x_bar", "xh_prev", "xh_next", "q", "g", "ws", "x0", "x", "x_bar_alt"):
        setattr(me, k, None)
    me.g = "G"
    real_ptr, real_stream = nv.ptr, nv.current_stream
    nv.ptr, nv.current_stream = (lambda t: t), (lambda device: None)          # no tensor, no device: the calls are only recorded
    me.device = None
    try:
        me._dual_kernel(0.5, 111)
        me._sweep_kernel(0.3, 0.5, 0.9, 111, 222, "GEO", "WS", None)
        out = type("O", (), {"data_ptr": lambda self: 333})()
        me._gap_kernel(None, None, 1.0, dict(xp=None, xn=None, qp=None, qn=None), out)
    finally:
        nv.ptr, nv.current_stream = real_ptr, real_stream
    assert [c[0] for c in rec.calls] == ["tv_cp_dual_hwtv", "tv_cp_hwtv_sweep", "tv_dual_gap_hwtv"]
    dual, sweep, gap = (c[1] for c in rec.calls)
    assert len(dual) == 12 and dual[5] == "G" and dual[6:9] == (0.5, 5.0, 2.0) and dual[9] == 111
    assert len(sweep) == 22 and sweep[9] == "G" and sweep[10:15] == (0.5, 5.0, 2.0, 0.3, 0.9) and sweep[15:18] == (0, 0, -1)
    assert len(gap) == 14 and gap[8] == "G" and gap[9:11] == (5.0, 2.0) and gap[11] == 333
