"""CPU-side checks of the flat streaming entry points (include/pytv4d.h: tv_sub, tv_dot, tv_cg_step1, tv_cg_step2, tv_cg_update,
tv_axpby, tv_cpop_p, tv_cpop_residual, tv_subgrad_step): every refusal is TV_E_ARG with a message, and is decided before anything
touches the device, so none of this needs a GPU.  The array arguments are host addresses that are never dereferenced."""
import ctypes

import pytest

TV_E_ARG = -1


@pytest.fixture(scope="module")
def nv():
    from pytv import _native
    return _native


@pytest.fixture(scope="module")
def P():
    """a non-NULL address for 'some array' (a host buffer, kept alive by the fixture; no entry point below reads it)"""
    buf = ctypes.create_string_buffer(64)
    return ctypes.addressof(buf), buf


def _geom(nv, dtype=0):
    g = nv.new_geom()
    g.nz, g.m, g.ny, g.nx, g.nz_global, g.z0 = 2, 1, 4, 8, 2, 0
    g.scheme, g.dtype = 0, dtype
    return g


def _refused(nv, rc):
    lib = nv.lib()
    assert rc == TV_E_ARG
    assert lib.tv_last_error() not in (None, b"")
    with pytest.raises(ValueError):
        nv.check(rc)


def _each_null(args, positions):
    """the argument list with one of the `positions` set to NULL, each in turn"""
    for k in positions:
        a = list(args)
        a[k] = None
        yield k, a


def test_raw_length_entry_points_refuse_bad_arguments(nv, P):
    lib, p = nv.lib(), P[0]
    calls = {
        "tv_sub": ([0, 8, p, p, p, None], (2, 3, 4)),
        "tv_cpop_p": ([0, 8, p, p, 0.5, None], (2, 3)),
        "tv_cpop_residual": ([0, 8, p, p, p, p, p, None], (2, 3, 4, 5, 6)),
    }
    for name, (args, arrays) in calls.items():
        fn = getattr(lib, name)
        for n in (-1, -2 ** 40):
            _refused(nv, fn(*(args[:1] + [n] + args[2:])))
        for dtype in (2, -1, 7):
            _refused(nv, fn(*([dtype] + args[1:])))
        for k, a in _each_null(args, arrays):
            _refused(nv, fn(*a))
            # ... whatever the length: a NULL array with n == 0 is refused too
            _refused(nv, fn(*(a[:1] + [0] + a[2:])))


def test_cpop_p_refuses_a_negative_or_nan_step(nv, P):
    lib, p = nv.lib(), P[0]
    for dtype in (0, 1):
        for sigma in (-1.0, -1e-300, float("-inf"), float("nan")):
            _refused(nv, lib.tv_cpop_p(dtype, 8, p, p, sigma, None))
            assert b"sigma_A" in lib.tv_last_error()
            _refused(nv, lib.tv_cpop_p(dtype, 0, p, p, sigma, None))


def test_zero_length_is_not_an_error(nv, P):
    """n == 0 returns 0 without a launch (tv_cpop_residual with n == 0 clears *fid on the device: test_gpu_flat_kernels.py)"""
    lib, p = nv.lib(), P[0]
    for dtype in (0, 1):
        assert lib.tv_sub(dtype, 0, p, p, p, None) == 0
        assert lib.tv_cpop_p(dtype, 0, p, p, 0.5, None) == 0
        assert lib.tv_cpop_p(dtype, 0, p, p, 0.0, None) == 0


def test_geometry_entry_points_refuse_null_arrays_and_unknown_dtypes(nv, P):
    lib, p = nv.lib(), P[0]
    # name: (arguments after the geometry, positions of the arrays that must not be NULL)
    calls = {
        "tv_dot": ([p, p, p, p, None], (0, 1, 2, 3)),
        "tv_cg_step1": ([p, p, p, p, p, p, p, p, None], (0, 1, 2, 3, 4, 5, 6, 7)),
        "tv_cg_step2": ([p, p, p, p, None], (0, 1, 2, 3)),
        "tv_cg_update": ([p, p, p, p, p, p, p, p, p, None], (0, 1, 2, 3, 4, 5, 8)),
        "tv_cg_update (no x0)": ([p, p, p, p, p, p, None, None, p, None], (0, 1, 2, 3, 4, 5, 8)),
        "tv_axpby": ([2.0, p, 3.0, p, p, p, p, p, None], (1,)),
        "tv_subgrad_step": ([p, p, p, 0.1, 2.0, p, p, None], (0, 1, 2, 5, 6)),
    }
    for name, (args, arrays) in calls.items():
        fn = getattr(lib, name.split()[0])
        for dtype in (0, 1):
            g = _geom(nv, dtype)
            for k, a in _each_null(args, arrays):
                _refused(nv, fn(ctypes.byref(g), *a))
        for dtype in (2, -1, 7):
            g = _geom(nv, dtype)
            _refused(nv, fn(ctypes.byref(g), *args))
            assert b"dtype" in lib.tv_last_error()
        _refused(nv, fn(None, *args))


def test_axpby_refuses_incomplete_argument_groups(nv, P):
    lib, p = nv.lib(), P[0]
    for dtype in (0, 1):
        g = ctypes.byref(_geom(nv, dtype))
        # "ref, dist2 and ws go together": (ref, dist2, ws)
        for ref, dist2, ws in ((p, None, p), (None, p, p), (p, p, None), (p, None, None), (None, p, None)):
            _refused(nv, lib.tv_axpby(g, 2.0, p, 3.0, p, ref, p, dist2, ws, None))
            assert b"go together" in lib.tv_last_error()
        # neither out nor ref: nothing to store and nothing to measure
        for ws in (p, None):
            _refused(nv, lib.tv_axpby(g, 2.0, p, 3.0, p, None, None, None, ws, None))
            _refused(nv, lib.tv_axpby(g, 2.0, p, 3.0, None, None, None, None, ws, None))


def test_cg_update_refuses_x0_without_a_place_for_the_fidelity(nv, P):
    lib, p = nv.lib(), P[0]
    for dtype in (0, 1):
        g = ctypes.byref(_geom(nv, dtype))
        _refused(nv, lib.tv_cg_update(g, p, p, p, p, p, p, p, None, p, None))
        assert b"fidelity" in lib.tv_last_error()
