"""CPU-side pins of the host launch layer (csrc/tv_host.h and the entry points built on it): the size of the reduction workspace, the
two-plane halo rule of the radius-2 entry points and the FIRST error each one-sweep entry point and each D / D^T epilogue entry point
reports for a bad call.  Every call
here returns from an argument check: the pointers (4096 and its multiples) are never followed and nothing is launched.  No GPU.

The literal tables were recorded from the library before the host layer was refactored (commit 9dfb747); they are the behaviour a
change of that layer has to keep.  EPI_FIRST_ERROR was recorded in the same way before the epilogue launch layer was folded into one pair
of runners (commit 649149b).

Not covered, on purpose:
  * the three "unsupported (scheme, M) ..." texts of the dispatchers: no entry point can reach them without a launch -- make_dg refuses
    unknown schemes, march_ok / subgrad_pass2_ok admit only the M that are instantiated, and the one-sweep / one-pass / streaming
    paths map every M > 8 to the windowed form;
  * "past the halo check" for tv_subgrad, tv_normal_op, tv_normal_op2, tv_cheb_step and tv_subgrad_fused: their halo check is their
    last argument check, so a call that passes it launches.  A NULL ``dots`` (or any other NULL array) does not help: those checks sit
    BEFORE the halo check, so failing one says nothing about whether the halo check was passed.  The slab tests of the GPU suite cover
    that side.
"""
import ctypes

import pytest

P = 4096                      # any non-NULL value
P2, P3, P4, P5, P6 = 2 * P, 3 * P, 4 * P, 5 * P, 6 * P


def _nv():
    from pytv import _native as nv
    return nv, nv.lib()


def _geom(nv, nz=4, m=1, ny=64, nx=64, nz_global=None, z0=0, scheme="hybrid", dtype=0, rz=1.0, rt=1.0, row_pitch=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = nz, m, ny, nx, (nz if nz_global is None else nz_global), z0
    g.scheme, g.dtype = nv.SCHEMES[scheme], dtype
    g.reg_z_over_reg, g.reg_time, g.factor_reg_static = rz, rt, 0.0
    g.row_pitch = row_pitch
    return g


# ---- tv_workspace_bytes -------------------------------------------------------------------------------------------------------------
FRAMES = ((8, 8), (100, 100), (64, 1024))
# (ny, nx, m) -> bytes at nz = 4; the same for fp32 / fp64 except where listed in WS_BYTES_F64, the same dense and pitched
WS_BYTES = {
    (8, 8, 1): 115200, (8, 8, 8): 139392, (8, 8, 16): 167040,
    (100, 100, 1): 194688, (100, 100, 8): 404352, (100, 100, 16): 643968,
    (64, 1024, 1): 251712, (64, 1024, 8): 594432, (64, 1024, 16): 986112,
}
WS_BYTES_F64 = {(64, 1024, 1): 398592, (64, 1024, 8): 1084032, (64, 1024, 16): 1867392}


def _pitch(nx, dtype):
    lane = 4 if dtype == 0 else 2
    return (nx + lane - 1) // lane * lane + lane


def _ws_cases():
    for ny, nx in FRAMES:
        for m in (1, 8, 16):
            for dtype in (0, 1):
                for pitched in (False, True):
                    yield ny, nx, m, dtype, pitched


def test_workspace_bytes_rules_and_recorded_values():
    nv, lib = _nv()
    for ny, nx, m, dtype, pitched in _ws_cases():
        sizes = []
        for nz in (1, 2, 4, 16, 64):
            g = _geom(nv, nz=nz, m=m, ny=ny, nx=nx, dtype=dtype, row_pitch=_pitch(nx, dtype) if pitched else 0)
            sizes.append(lib.tv_workspace_bytes(ctypes.byref(g)))
        case = (ny, nx, m, dtype, pitched)
        assert all(s > 0 and s % 8 == 0 for s in sizes), case
        assert sizes == sorted(sizes), case                                  # monotone in nz
        want = WS_BYTES_F64.get((ny, nx, m), WS_BYTES[(ny, nx, m)]) if dtype == 1 else WS_BYTES[(ny, nx, m)]
        assert sizes[2] == want, (case, sizes[2])
    bad = _geom(nv, nx=0)
    assert lib.tv_workspace_bytes(ctypes.byref(bad)) == 0
    bad = _geom(nv)
    bad.abi_version = 4
    assert lib.tv_workspace_bytes(ctypes.byref(bad)) == 0
    bad = _geom(nv, row_pitch=65)                                            # not a multiple of 16 bytes
    assert lib.tv_workspace_bytes(ctypes.byref(bad)) == 0


# ---- the two-plane halo rule ----------------------------------------------------------------------------------------------------------
def _halo_calls(lib, g, xp, xn, step=1.0):
    """name -> call of each radius-2 entry point on geometry g with the halo pointers (xp, xn); everything else is non-NULL and distinct"""
    G = ctypes.byref(g)
    return {
        "tv_subgrad": lambda: lib.tv_subgrad(G, P, xp, xn, P2, P3, P4, P5, None),
        "tv_normal_op": lambda: lib.tv_normal_op(G, P, xp, xn, 1.0, P2, P4, P5, None),
        "tv_normal_op2": lambda: lib.tv_normal_op2(G, P, xp, xn, 1.0, P3, P2, None, P4, P5, None),
        "tv_cheb_step": lambda: lib.tv_cheb_step(G, P, xp, xn, 1.0, P3, None, 0.0, None, None, 1.0, 0.0, P2, P4, P5, None),
        "tv_subgrad_fused": lambda: lib.tv_subgrad_fused(G, P, xp, xn, P2, P4, P5, None),
        "tv_subgrad_fused_norms": lambda: lib.tv_subgrad_fused_norms(G, P, xp, xn, P2, P3, P4, P5, None),
        "tv_subgrad_step_fused": lambda: lib.tv_subgrad_step_fused(G, P, xp, xn, P3, P2, step, 5.0, P4, P6, P5, None),
    }


HALO_TEXT = " on a slab needs two halo planes on each interior side"


@pytest.mark.parametrize("z0, missing", [(3, "prev"), (3, "next"), (0, "next"), (6, "prev")])
def test_two_plane_halo_rule(z0, missing):
    """interior slab: both sides are needed; first slab: the next side; last slab: the previous side -- whatever the scheme's own radius"""
    nv, lib = _nv()
    for scheme in ("hybrid", "upwind"):
        g = _geom(nv, nz=3, m=1, ny=8, nx=8, nz_global=9, z0=z0, scheme=scheme, rz=1.0, rt=0.0)
        # the side that is not under test is given where the slab has it, and left NULL at the ends of the volume
        xp = None if (missing == "prev" or z0 == 0) else P6
        xn = None if (missing == "next" or z0 == 6) else P6
        for name, call in _halo_calls(lib, g, xp, xn).items():
            assert call() == -2, (name, scheme)
            assert lib.tv_last_error().decode() == name + HALO_TEXT, (name, scheme)


def test_no_halo_rule_without_a_z_term():
    """reg_z_over_reg = 0: no halo is asked for.  Only tv_subgrad_step_fused has an argument check behind its halo check (the module
    docstring says why the others are not called): with step = 0 it reports that check, fp32 and fp64"""
    nv, lib = _nv()
    want = {
        0: "the one-pass sub-gradient kernel needs step * lambda >= 1e-6 and frames below 2^31 bytes: use tv_subgrad + tv_subgrad_step",
        1: "the fp64 one-pass descent step needs step * lambda >= 1e-6: use tv_subgrad + tv_subgrad_step",
    }
    for dtype in (0, 1):
        g = _geom(nv, nz=3, m=1, ny=8, nx=8, nz_global=9, z0=3, dtype=dtype, rz=0.0, rt=0.0)
        call = _halo_calls(lib, g, None, None, step=0.0)["tv_subgrad_step_fused"]
        assert call() == -1
        assert lib.tv_last_error().decode() == want[dtype]
        g = _geom(nv, nz=3, m=1, ny=8, nx=8, nz_global=9, z0=3, dtype=dtype, rz=1.0, rt=0.0)      # and with the z term the halo comes first
        assert _halo_calls(lib, g, None, None, step=0.0)["tv_subgrad_step_fused"]() == -2


# ---- first error of the one-sweep entry points -----------------------------------------------------------------------------------------
NULL, UNSUP = "NULL array", "geometry not supported by the one-sweep path"


def _sweep_calls(lib, g):
    """(entry point, kind) -> call.  kinds: null (one array NULL), alias, nx32 (every argument fine, the geometry is not)"""
    G = ctypes.byref(g)

    def cp_sweep(x_in=P, q_in=P2, q_out=P2, x0=P3, p=P4, x_out=P5, flags=0):
        return lib.tv_cp_sweep(G, x_in, None, None, q_in, q_out, x0, p, x_out, 0.3, 5.0, 0.3, 1.0, flags, 0, -1, P6, P6 + 64, P6 + 4096, None)

    def cp_fused(x_in=P, q=P2, x_out=P5):
        return lib.tv_cp_fused(G, x_in, None, None, q, P3, P4, x_out, 0.3, 5.0, 0.3, 1.0, 0, -1, P6, P6 + 64, P6 + 4096, None)

    def cp_fixup(q=P2, fid=P6):
        return lib.tv_cp_fixup(G, q, None, None, P5, P3, 0.3, 0, -1, fid, P6 + 4096, None)

    def admm_sweep(x=P, u=P2, t=P3, x0=P4, r=P5):
        return lib.tv_admm_sweep(G, x, None, None, u, u, t, x0, r, 0.1, 1.0, 0, 0, -1, P6, P6 + 64, P6 + 4096, None)

    def admm_fixup(t=P3, rr=P6):
        return lib.tv_admm_fixup(G, t, None, None, P5, 1.0, 0, -1, rr, P6 + 4096, None)

    def cpop_fused(x_in=P, q=P2, atp=P3, x_out=P5):
        return lib.tv_cpop_fused(G, x_in, None, None, q, atp, x_out, 0.3, 5.0, 0.3, 0, -1, P6, P6 + 4096, None)

    def cpop_fixup(q=P2, ws=P6 + 4096):
        return lib.tv_cpop_fixup(G, q, None, None, P5, 0.3, 0, -1, ws, None)

    return {
        ("tv_cp_sweep", "null"): lambda: cp_sweep(q_in=None),
        ("tv_cp_sweep", "null2"): lambda: cp_sweep(x0=None),
        ("tv_cp_sweep", "alias"): lambda: cp_sweep(x_out=P),
        ("tv_cp_sweep", "flag"): lambda: cp_sweep(flags=8),
        ("tv_cp_sweep", "flag2"): lambda: cp_sweep(flags=2),
        ("tv_cp_sweep", "nx32"): cp_sweep,
        ("tv_cp_fused", "null"): lambda: cp_fused(q=None),
        ("tv_cp_fused", "alias"): lambda: cp_fused(x_out=P),
        ("tv_cp_fused", "nx32"): cp_fused,
        ("tv_cp_fixup", "null"): lambda: cp_fixup(fid=None),
        ("tv_cp_fixup", "nx32"): cp_fixup,
        ("tv_admm_sweep", "null"): lambda: admm_sweep(x0=None),
        ("tv_admm_sweep", "alias"): lambda: admm_sweep(t=P2),             # u == t
        ("tv_admm_sweep", "alias2"): lambda: admm_sweep(r=P),             # r == x
        ("tv_admm_sweep", "nx32"): admm_sweep,
        ("tv_admm_fixup", "null"): lambda: admm_fixup(rr=None),
        ("tv_admm_fixup", "null2"): lambda: admm_fixup(t=None),
        ("tv_admm_fixup", "nx32"): admm_fixup,
        ("tv_cpop_fused", "null"): lambda: cpop_fused(atp=None),
        ("tv_cpop_fused", "alias"): lambda: cpop_fused(x_out=P),
        ("tv_cpop_fused", "alias2"): lambda: cpop_fused(x_out=P3),        # atp == x_out
        ("tv_cpop_fused", "nx32"): cpop_fused,
        ("tv_cpop_fixup", "null"): lambda: cpop_fixup(ws=None),
        ("tv_cpop_fixup", "null2"): lambda: cpop_fixup(q=None),
        ("tv_cpop_fixup", "nx32"): cpop_fixup,
    }


# the fix-ups check no aliasing (their callers pass the sweep's own buffers), so they have no "alias" row
FIRST_ERROR = {
    ("tv_cp_sweep", "null"): NULL, ("tv_cp_sweep", "null2"): NULL,
    ("tv_cp_sweep", "alias"): "x_in and x_out must be different buffers (ping-pong)",
    ("tv_cp_sweep", "flag"): "tv_cp_sweep: unknown flag", ("tv_cp_sweep", "flag2"): "tv_cp_sweep: TV_CP_FID_BOTH extends TV_CP_FID_OF_INPUT",
    ("tv_cp_sweep", "nx32"): UNSUP,
    ("tv_cp_fused", "null"): NULL, ("tv_cp_fused", "alias"): "x_in and x_out must be different buffers (ping-pong)", ("tv_cp_fused", "nx32"): UNSUP,
    ("tv_cp_fixup", "null"): NULL, ("tv_cp_fixup", "nx32"): UNSUP,
    ("tv_admm_sweep", "null"): NULL, ("tv_admm_sweep", "alias"): "u and t must be different arrays",
    ("tv_admm_sweep", "alias2"): "r must not alias x or x0", ("tv_admm_sweep", "nx32"): UNSUP,
    ("tv_admm_fixup", "null"): NULL, ("tv_admm_fixup", "null2"): NULL, ("tv_admm_fixup", "nx32"): UNSUP,
    ("tv_cpop_fused", "null"): NULL, ("tv_cpop_fused", "alias"): "x_out must be a buffer of its own (ping-pong)",
    ("tv_cpop_fused", "alias2"): "x_out must be a buffer of its own (ping-pong)", ("tv_cpop_fused", "nx32"): UNSUP,
    ("tv_cpop_fixup", "null"): NULL, ("tv_cpop_fixup", "null2"): NULL, ("tv_cpop_fixup", "nx32"): UNSUP,
}


@pytest.mark.parametrize("dtype", [0, 1])
def test_first_error_of_the_one_sweep_entry_points(dtype):
    nv, lib = _nv()
    good, narrow = _geom(nv, dtype=dtype), _geom(nv, nx=32, dtype=dtype)
    assert lib.tv_cp_fused_supported(ctypes.byref(good)) == 1 and lib.tv_cp_fused_supported(ctypes.byref(narrow)) == 0
    calls, calls32 = _sweep_calls(lib, good), _sweep_calls(lib, narrow)
    assert set(calls) == set(FIRST_ERROR)
    for key, text in FIRST_ERROR.items():
        call = calls32[key] if key[1] == "nx32" else calls[key]
        assert call() == -1, key
        assert lib.tv_last_error().decode() == text, key
    # with every argument fine, a bad geometry struct is what is reported
    bad = _geom(nv)
    bad.abi_version = 4
    for key, call in _sweep_calls(lib, bad).items():
        if key[1] == "nx32":
            assert call() == -1 and lib.tv_last_error().decode().startswith("tv_geom was built against another version"), key


# ---- first error of the D / D^T epilogue entry points ---------------------------------------------------------------------------------
# Ordered parameters after the geometry (the stream, always NULL, comes last): pointers default to distinct non-NULL values, the halo
# planes to NULL.  Every call below is made on an INTERIOR slab (3 x 1 x 8 x 8 at z0 = 3 of 9 planes, with a z term) whose halo planes are
# missing unless the case says otherwise, so a call that passes every argument check still returns from the halo check -- the last check
# before the launch -- and never touches the device.  That also pins the order "arguments before halos", and which scalars an entry point
# does NOT check (tv_cp_dual takes lambda = +inf, nobody looks at sigma_D, sigma_A or thresh).
HUBER_FID, RESIDUAL = 2, 1
_X = [("c", P), ("prev", None), ("next", None)]                  # the centre array of the stencil and its halo planes
EPI_PARAMS = {
    "tv_cp_dual": _X + [("q", P2), ("sigma_D", 0.3), ("lambda", 5.0), ("out", P3), ("ws", P4)],
    "tv_cp_dual_huber": _X + [("q", P2), ("sigma_D", 0.3), ("lambda", 5.0), ("alpha", 0.1), ("out", P3), ("ws", P4)],
    "tv_admm_zu": _X + [("z", P2), ("u", P3), ("thresh", 0.1), ("out", P4), ("ws", P5)],
    "tv_admm_tu": _X + [("z", P2), ("u", P3), ("thresh", 0.1), ("out", P4), ("ws", P5)],
    "tv_cp_primal": _X + [("x", P2), ("x0", P3), ("p", P4), ("tau", 0.3), ("sigma_A", 1.0), ("out", P5), ("ws", P6)],
    "tv_cp_primal_accel": _X + [("x", P2), ("x_bar", P3), ("x0", P4), ("tau", 0.3), ("theta", 0.5), ("out", P5), ("ws", P6)],
    "tv_cp_primal_prox": _X + [("x", P2), ("x_bar", P3), ("x0", P4), ("fidelity", HUBER_FID), ("delta", 0.5), ("tau", 0.3), ("theta", 0.5),
                               ("flags", 0), ("out", P5), ("ws", P6)],
    "tv_cp_primal_kl": _X + [("x", P2), ("x_bar", P3), ("x0", P4), ("tau", 0.3), ("theta", 0.5), ("flags", 0), ("out", P5), ("ws", P6)],
}
# (entry point, flags): the prox and KL entries in step mode and in residual mode
EPI_ENTRIES = [(n, None) for n in EPI_PARAMS if "flags" not in dict(EPI_PARAMS[n])] + [(n, f) for n in ("tv_cp_primal_prox", "tv_cp_primal_kl")
                                                                                        for f in (0, RESIDUAL)]
BAD_SCALARS = (("0", 0.0), ("neg", -1.0), ("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")))
ALL_SCHEMES = ("upwind", "downwind", "central", "hybrid")


def _halo_needed(name, scheme, side):
    """check_x_halos / check_y_halos: the forward stencil of `upwind` looks at the next plane only, its adjoint at the previous one only"""
    forward = name in ("tv_cp_dual", "tv_cp_dual_huber", "tv_admm_zu", "tv_admm_tu")
    return scheme != {(True, "prev"): "upwind", (True, "next"): "downwind", (False, "prev"): "downwind", (False, "next"): "upwind"}[(forward, side)]


def _epi_cases(name, flags):
    """case -> (scheme, overrides).  Every case holds at least one fault that the entry point reports: none of them launches."""
    params = dict(EPI_PARAMS[name])
    arrays = [k for k, v in EPI_PARAMS[name] if isinstance(v, int) and k not in ("fidelity", "flags")]
    scalars = [k for k, v in EPI_PARAMS[name] if isinstance(v, float)]
    cases = {}
    for a in arrays:
        cases["null:" + a] = ("hybrid", {a: None})
    for s in scalars:
        for tag, v in BAD_SCALARS:
            cases["%s=%s" % (s, tag)] = ("hybrid", {s: v})
    if "x_bar" in params:
        cases["x==x_bar"] = ("hybrid", {"x_bar": params["x"]})
    if "flags" in params:
        cases["flags=2"], cases["flags=4|mode"] = ("hybrid", {"flags": 2}), ("hybrid", {"flags": 4 | flags})
        cases["flag+null"] = ("hybrid", {"flags": 2, "c": None})              # two faults: the flag comes before the NULL
    if "fidelity" in params:
        cases["fidelity=-1"], cases["fidelity=3"] = ("hybrid", {"fidelity": -1}), ("hybrid", {"fidelity": 3})
        cases["fidelity+flag"] = ("hybrid", {"fidelity": 3, "flags": 2})
    for s in scalars:
        cases["null+%s" % s] = ("hybrid", {"c": None, s: -1.0})               # two faults: the NULL comes before the scalar
    if "x_bar" in params:
        cases["alias+tau"] = ("hybrid", {"x_bar": params["x"], "tau": -1.0})
    # halos (every scalar case above is "scalar + missing halo" already): one side missing where the scheme needs that side -- where it does
    # not, the call would pass -- and both missing, for every scheme
    for scheme in ALL_SCHEMES:
        for side, other in (("prev", "next"), ("next", "prev")):
            if _halo_needed(name, scheme, side):
                cases["halo:%s:%s" % (scheme, side)] = (scheme, {other: P6})
        cases["halo:%s:both" % scheme] = (scheme, {})
    return cases


def _epi_call(nv, lib, name, flags, scheme, dtype, overrides):
    g = _geom(nv, nz=3, m=1, ny=8, nx=8, nz_global=9, z0=3, scheme=scheme, dtype=dtype, rz=1.0, rt=0.0)
    a = dict(EPI_PARAMS[name])
    if flags is not None:
        a["flags"] = flags
    a.update(overrides)
    assert set(a) == set(dict(EPI_PARAMS[name]))
    rc = getattr(lib, name)(ctypes.byref(g), *[a[k] for k, _ in EPI_PARAMS[name]], None)
    return rc, lib.tv_last_error().decode()


# the texts, by the short names the table below uses; the return code is -2 for the two halo texts and -1 for everything else
EPI_TEXT = {
    "NULL": "NULL array",
    "prev_x": "previous-slab halo plane required", "next_x": "next-slab halo plane required",
    "prev_y": "previous-slab gradient halo required", "next_y": "next-slab gradient halo required",
    "lambda": "lambda must be > 0", "lambda_f": "lambda must be a finite number > 0",
    "alpha": "alpha must be a finite number > 0 (alpha = 0 is plain TV: tv_cp_dual)",
    "sigma_D": "sigma_D must be a finite number > 0",
    "alias": "x and x_bar must be different arrays",
    "tau": "tau must be a finite number > 0", "theta": "theta must be a finite number in [0, 1]", "delta": "delta must be a finite number > 0",
    "fid": "unknown fidelity", "flag": "unknown flag bits",
}
EPI_HALO_TEXTS = ("prev_x", "next_x", "prev_y", "next_y")
# (entry point, flags) -> case -> text; recorded, the same for fp32 and fp64
EPI_FIRST_ERROR = {
    ("tv_cp_dual", None): {
        "null:c": "NULL", "null:q": "NULL", "null:out": "NULL", "null:ws": "NULL", "sigma_D=0": "prev_x", "sigma_D=neg": "prev_x",
        "sigma_D=nan": "prev_x", "sigma_D=+inf": "prev_x", "sigma_D=-inf": "prev_x", "lambda=0": "lambda", "lambda=neg": "lambda",
        "lambda=nan": "lambda", "lambda=+inf": "prev_x", "lambda=-inf": "lambda", "null+sigma_D": "NULL", "null+lambda": "NULL",
        "halo:upwind:next": "next_x", "halo:upwind:both": "next_x", "halo:downwind:prev": "prev_x", "halo:downwind:both": "prev_x",
        "halo:central:prev": "prev_x", "halo:central:next": "next_x", "halo:central:both": "prev_x", "halo:hybrid:prev": "prev_x",
        "halo:hybrid:next": "next_x", "halo:hybrid:both": "prev_x",
    },
    ("tv_cp_dual_huber", None): {
        "null:c": "NULL", "null:q": "NULL", "null:out": "NULL", "null:ws": "NULL", "sigma_D=0": "sigma_D", "sigma_D=neg": "sigma_D",
        "sigma_D=nan": "sigma_D", "sigma_D=+inf": "sigma_D", "sigma_D=-inf": "sigma_D", "lambda=0": "lambda_f", "lambda=neg": "lambda_f",
        "lambda=nan": "lambda_f", "lambda=+inf": "lambda_f", "lambda=-inf": "lambda_f", "alpha=0": "alpha", "alpha=neg": "alpha",
        "alpha=nan": "alpha", "alpha=+inf": "alpha", "alpha=-inf": "alpha", "null+sigma_D": "NULL", "null+lambda": "NULL",
        "null+alpha": "NULL", "halo:upwind:next": "next_x", "halo:upwind:both": "next_x", "halo:downwind:prev": "prev_x",
        "halo:downwind:both": "prev_x", "halo:central:prev": "prev_x", "halo:central:next": "next_x", "halo:central:both": "prev_x",
        "halo:hybrid:prev": "prev_x", "halo:hybrid:next": "next_x", "halo:hybrid:both": "prev_x",
    },
    ("tv_admm_zu", None): {
        "null:c": "NULL", "null:z": "NULL", "null:u": "NULL", "null:out": "NULL", "null:ws": "NULL", "thresh=0": "prev_x",
        "thresh=neg": "prev_x", "thresh=nan": "prev_x", "thresh=+inf": "prev_x", "thresh=-inf": "prev_x", "null+thresh": "NULL",
        "halo:upwind:next": "next_x", "halo:upwind:both": "next_x", "halo:downwind:prev": "prev_x", "halo:downwind:both": "prev_x",
        "halo:central:prev": "prev_x", "halo:central:next": "next_x", "halo:central:both": "prev_x", "halo:hybrid:prev": "prev_x",
        "halo:hybrid:next": "next_x", "halo:hybrid:both": "prev_x",
    },
    ("tv_admm_tu", None): {
        "null:c": "NULL", "null:z": "NULL", "null:u": "NULL", "null:out": "NULL", "null:ws": "NULL", "thresh=0": "prev_x",
        "thresh=neg": "prev_x", "thresh=nan": "prev_x", "thresh=+inf": "prev_x", "thresh=-inf": "prev_x", "null+thresh": "NULL",
        "halo:upwind:next": "next_x", "halo:upwind:both": "next_x", "halo:downwind:prev": "prev_x", "halo:downwind:both": "prev_x",
        "halo:central:prev": "prev_x", "halo:central:next": "next_x", "halo:central:both": "prev_x", "halo:hybrid:prev": "prev_x",
        "halo:hybrid:next": "next_x", "halo:hybrid:both": "prev_x",
    },
    ("tv_cp_primal", None): {
        "null:c": "NULL", "null:x": "NULL", "null:x0": "NULL", "null:p": "NULL", "null:out": "NULL", "null:ws": "NULL", "tau=0": "prev_y",
        "tau=neg": "prev_y", "tau=nan": "prev_y", "tau=+inf": "prev_y", "tau=-inf": "prev_y", "sigma_A=0": "prev_y",
        "sigma_A=neg": "prev_y", "sigma_A=nan": "prev_y", "sigma_A=+inf": "prev_y", "sigma_A=-inf": "prev_y", "null+tau": "NULL",
        "null+sigma_A": "NULL", "halo:upwind:prev": "prev_y", "halo:upwind:both": "prev_y", "halo:downwind:next": "next_y",
        "halo:downwind:both": "next_y", "halo:central:prev": "prev_y", "halo:central:next": "next_y", "halo:central:both": "prev_y",
        "halo:hybrid:prev": "prev_y", "halo:hybrid:next": "next_y", "halo:hybrid:both": "prev_y",
    },
    ("tv_cp_primal_accel", None): {
        "null:c": "NULL", "null:x": "NULL", "null:x_bar": "NULL", "null:x0": "NULL", "null:out": "NULL", "null:ws": "NULL", "tau=0": "tau",
        "tau=neg": "tau", "tau=nan": "tau", "tau=+inf": "tau", "tau=-inf": "tau", "theta=0": "prev_y", "theta=neg": "theta",
        "theta=nan": "theta", "theta=+inf": "theta", "theta=-inf": "theta", "x==x_bar": "alias", "null+tau": "NULL", "null+theta": "NULL",
        "alias+tau": "alias", "halo:upwind:prev": "prev_y", "halo:upwind:both": "prev_y", "halo:downwind:next": "next_y",
        "halo:downwind:both": "next_y", "halo:central:prev": "prev_y", "halo:central:next": "next_y", "halo:central:both": "prev_y",
        "halo:hybrid:prev": "prev_y", "halo:hybrid:next": "next_y", "halo:hybrid:both": "prev_y",
    },
    ("tv_cp_primal_prox", 0): {
        "null:c": "NULL", "null:x": "NULL", "null:x_bar": "NULL", "null:x0": "NULL", "null:out": "NULL", "null:ws": "NULL",
        "delta=0": "delta", "delta=neg": "delta", "delta=nan": "delta", "delta=+inf": "delta", "delta=-inf": "delta", "tau=0": "tau",
        "tau=neg": "tau", "tau=nan": "tau", "tau=+inf": "tau", "tau=-inf": "tau", "theta=0": "prev_y", "theta=neg": "theta",
        "theta=nan": "theta", "theta=+inf": "theta", "theta=-inf": "theta", "x==x_bar": "alias", "flags=2": "flag", "flags=4|mode": "flag",
        "flag+null": "flag", "fidelity=-1": "fid", "fidelity=3": "fid", "fidelity+flag": "fid", "null+delta": "NULL", "null+tau": "NULL",
        "null+theta": "NULL", "alias+tau": "alias", "halo:upwind:prev": "prev_y", "halo:upwind:both": "prev_y",
        "halo:downwind:next": "next_y", "halo:downwind:both": "next_y", "halo:central:prev": "prev_y", "halo:central:next": "next_y",
        "halo:central:both": "prev_y", "halo:hybrid:prev": "prev_y", "halo:hybrid:next": "next_y", "halo:hybrid:both": "prev_y",
    },
    ("tv_cp_primal_prox", 1): {
        "null:c": "NULL", "null:x": "NULL", "null:x_bar": "prev_y", "null:x0": "NULL", "null:out": "NULL", "null:ws": "NULL",
        "delta=0": "delta", "delta=neg": "delta", "delta=nan": "delta", "delta=+inf": "delta", "delta=-inf": "delta", "tau=0": "tau",
        "tau=neg": "tau", "tau=nan": "tau", "tau=+inf": "tau", "tau=-inf": "tau", "theta=0": "prev_y", "theta=neg": "prev_y",
        "theta=nan": "prev_y", "theta=+inf": "prev_y", "theta=-inf": "prev_y", "x==x_bar": "alias", "flags=2": "flag",
        "flags=4|mode": "flag", "flag+null": "flag", "fidelity=-1": "fid", "fidelity=3": "fid", "fidelity+flag": "fid",
        "null+delta": "NULL", "null+tau": "NULL", "null+theta": "NULL", "alias+tau": "alias", "halo:upwind:prev": "prev_y",
        "halo:upwind:both": "prev_y", "halo:downwind:next": "next_y", "halo:downwind:both": "next_y", "halo:central:prev": "prev_y",
        "halo:central:next": "next_y", "halo:central:both": "prev_y", "halo:hybrid:prev": "prev_y", "halo:hybrid:next": "next_y",
        "halo:hybrid:both": "prev_y",
    },
    ("tv_cp_primal_kl", 0): {
        "null:c": "NULL", "null:x": "NULL", "null:x_bar": "NULL", "null:x0": "NULL", "null:out": "NULL", "null:ws": "NULL", "tau=0": "tau",
        "tau=neg": "tau", "tau=nan": "tau", "tau=+inf": "tau", "tau=-inf": "tau", "theta=0": "prev_y", "theta=neg": "theta",
        "theta=nan": "theta", "theta=+inf": "theta", "theta=-inf": "theta", "x==x_bar": "alias", "flags=2": "flag", "flags=4|mode": "flag",
        "flag+null": "flag", "null+tau": "NULL", "null+theta": "NULL", "alias+tau": "alias", "halo:upwind:prev": "prev_y",
        "halo:upwind:both": "prev_y", "halo:downwind:next": "next_y", "halo:downwind:both": "next_y", "halo:central:prev": "prev_y",
        "halo:central:next": "next_y", "halo:central:both": "prev_y", "halo:hybrid:prev": "prev_y", "halo:hybrid:next": "next_y",
        "halo:hybrid:both": "prev_y",
    },
    ("tv_cp_primal_kl", 1): {
        "null:c": "NULL", "null:x": "NULL", "null:x_bar": "prev_y", "null:x0": "NULL", "null:out": "NULL", "null:ws": "NULL",
        "tau=0": "tau", "tau=neg": "tau", "tau=nan": "tau", "tau=+inf": "tau", "tau=-inf": "tau", "theta=0": "prev_y",
        "theta=neg": "prev_y", "theta=nan": "prev_y", "theta=+inf": "prev_y", "theta=-inf": "prev_y", "x==x_bar": "alias",
        "flags=2": "flag", "flags=4|mode": "flag", "flag+null": "flag", "null+tau": "NULL", "null+theta": "NULL", "alias+tau": "alias",
        "halo:upwind:prev": "prev_y", "halo:upwind:both": "prev_y", "halo:downwind:next": "next_y", "halo:downwind:both": "next_y",
        "halo:central:prev": "prev_y", "halo:central:next": "next_y", "halo:central:both": "prev_y", "halo:hybrid:prev": "prev_y",
        "halo:hybrid:next": "next_y", "halo:hybrid:both": "prev_y",
    },
}


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name, flags", EPI_ENTRIES)
def test_first_error_of_the_epilogue_entry_points(name, flags, dtype):
    nv, lib = _nv()
    cases, want = _epi_cases(name, flags), EPI_FIRST_ERROR[(name, flags)]
    assert set(cases) == set(want)
    for case, (scheme, overrides) in cases.items():
        rc, text = _epi_call(nv, lib, name, flags, scheme, dtype, overrides)
        code = want[case]
        assert (rc, text) == (-2 if code in EPI_HALO_TEXTS else -1, EPI_TEXT[code]), (case, rc, text)
