"""CPU-side pins of the host launch layer (csrc/tv_host.h and the entry points built on it): the size of the reduction workspace, the
two-plane halo rule of the radius-2 entry points and the FIRST error each one-sweep entry point reports for a bad call.  Every call
here returns from an argument check: the pointers (4096 and its multiples) are never followed and nothing is launched.  No GPU.

The literal tables were recorded from the library before the host layer was refactored (commit 9dfb747); they are the behaviour a
change of that layer has to keep.

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
