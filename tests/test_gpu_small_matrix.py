"""The persistent small-volume loops (csrc/tv_small.hip: tv_small_cp, tv_small_subgrad_descent) on what they accept beyond the plain
dense volume of test_gpu_small.py: weight volumes and weight maps, boolean masks with the reference's defaults, pitched state, runs that
cross launch boundaries, non-default step parameters, a workspace whose epoch counter wraps around, and non-finite numbers.

Every solver is built with ``persistent=True`` and checked with ``assert solver.small``: which path runs does not depend on options other
modules set for the whole process.  The reference is the fp64 oracle on the up-cast input; the inputs (and weights) are fp32 values, so
one oracle run serves both dtypes.  Tolerances are test_gpu_small.py's: fp64 1e-10 (CP) / 1e-9 (descent), fp32 1e-5 / 2e-5 relative on the
loss, with its atol on the iterate."""
import hashlib

import numpy as np
import pytest

from conftest import SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

REG, STEP = 25.0, 5e-3
# Runs past ~130 iterations take the descent with a smaller step.  With step 5e-3 the fixed-step sub-gradient iteration is ill-conditioned there
# for the one-sided stencils: the kinks of |Dx| make it chaotic, and a 1e-14 relative perturbation of the INPUT moves the fp64 oracle's own
# loss by up to 3e-4 (upwind, (3, 1, 8, 12), 257 iterations) -- no implementation can be held to 1e-9 against it.  With step 1e-3 the same
# perturbation moves it by < 1e-13 on every case below, so the module's tolerances keep their meaning.
STEP_LONG = 1e-3
DTYPES = (np.float64, np.float32)
TOL = {("cp", np.float64): (1e-10, 1e-9), ("cp", np.float32): (1e-5, 2e-3),
       ("sg", np.float64): (1e-9, 1e-8), ("sg", np.float32): (2e-5, 5e-3)}

# the workspace layout of csrc/tv_small.hip:45-51,110 (kFlagStride, kMaxSmallBlocks, small_epoch_base, small_abort_word), in 32-bit words:
# one 128-byte flag line per launched block (word 0: the block's phase counter), then the epoch word, then the abort word
K_FLAG_STRIDE = 32
K_MAX_SMALL_BLOCKS = 8192
EPOCH_WORD = K_MAX_SMALL_BLOCKS * K_FLAG_STRIDE
ABORT_WORD = EPOCH_WORD + 1


@pytest.fixture(scope="module")
def pytv():
    import pytv
    return pytv


def _set_form(nv, form):
    """as test_gpu_small._set_form: registers (the default order), streamedN (TV_SMALL_SITES = N), generic (TV_SMALL_GENERIC)"""
    nv.set_option("TV_SMALL_GENERIC", 1 if form == "generic" else None)
    nv.set_option("TV_SMALL_SITES", int(form[-1]) if form and form.startswith("streamed") else None)


class _form:
    def __init__(self, form):
        from pytv import _native as nv
        self.nv, self.form = nv, form

    def __enter__(self):
        _set_form(self.nv, self.form)

    def __exit__(self, *exc):
        _set_form(self.nv, None)


def _input(shape, seed=5):
    """the noisy phantom of test_gpu_small.py, rounded to fp32 values (exact in both dtypes), as fp64"""
    truth = orc.phantom(shape, seed=seed, dtype=np.float64)
    rng = np.random.RandomState(seed)
    return (truth + 100.0 * rng.rand(*shape)).astype(np.float32).astype(np.float64)


def _digest(v):
    if isinstance(v, np.ndarray):
        return (v.shape, str(v.dtype), hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, dict):
        return tuple(sorted((k, _digest(x)) for k, x in v.items()))
    return v


_ORACLE = {}


def _oracle(kind, x0, n, scheme, kw, reg=REG, step=STEP, cp_kw=None):
    """fp64 oracle run (memoised: the forms and dtypes of one case share it)"""
    cp_kw = cp_kw or {}
    key = (kind, _digest(x0), n, scheme, _digest(kw), reg, step, _digest(cp_kw))
    if key not in _ORACLE:
        with np.errstate(invalid="ignore", over="ignore"):
            if kind == "cp":
                _ORACLE[key] = orc.chambolle_pock(x0, n, reg, scheme=scheme, **kw, **cp_kw)
            else:
                _ORACLE[key] = orc.subgradient_descent(x0, n, reg, step, scheme=scheme, **kw)
    return _ORACLE[key]


def _solver(pytv, kind, x0, dtype, scheme, kw, pitch=None, reg=REG, step=STEP, cp_kw=None, persistent=True):
    import torch
    t = torch.as_tensor(np.asarray(x0).astype(dtype)).cuda()
    if kind == "cp":
        extra = dict(fused=False) if persistent is False else {}
        s = pytv.solvers.ChambollePock(t, reg, scheme=scheme, persistent=persistent, pitch=pitch, **kw, **(cp_kw or {}), **extra)
    else:
        extra = dict(one_pass=False) if persistent is False else {}
        s = pytv.solvers.SubgradientDescent(t, reg, step, scheme=scheme, persistent=persistent, pitch=pitch, **kw, **extra)
    assert s.small == (persistent is True)
    return s


def _check(pytv, kind, x0, n, scheme, kw, dtypes=DTYPES, what="", **skw):
    """persistent run of n iterations == oracle (loss and iterate), in each dtype; returns the last solver"""
    wx, wloss = _oracle(kind, x0, n, scheme, kw, **{k: v for k, v in skw.items() if k in ("reg", "step", "cp_kw")})
    s = None
    for dtype in dtypes:
        rtol, atol = TOL[(kind, dtype)]
        s = _solver(pytv, kind, x0, dtype, scheme, kw, **skw)
        loss = s.run(n)
        msg = "%s %s %s %s n=%d %s" % (kind, scheme, np.dtype(dtype).name, x0.shape, n, what)
        np.testing.assert_allclose(loss, wloss, rtol=rtol, err_msg=msg)
        np.testing.assert_allclose(s.result().cpu().numpy(), wx, rtol=rtol, atol=atol, err_msg=msg)
    return s


def _pads_zero(t):
    """every storage element of the strided view t that is NOT one of its elements is zero (test_gpu_pitch._pads_zero)"""
    n = 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride()))
    flat = t.as_strided((n,), (1,))
    total = flat.double().abs().sum().item()
    inside = t.double().abs().sum().item()
    return abs(total - inside) <= 1e-9 * max(1.0, total)


# ---- 1. weight volume: the generic persistent form -------------------------------------------------------------------------------------
WV_SHAPES = [((3, 2, 7, 13), 140), ((4, 1, 9, 16), 24), ((2, 10, 6, 12), 24)]      # ragged Nx (and a run of more than SMALL_BLOCK), M = 1, M > 8


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,n", WV_SHAPES)
def test_weight_volume_generic_form(pytv, scheme, shape, n):
    """a per-voxel mask_static volume can only take the generic form (tv_small.hip small_plan_flat): W varies along z and t, zero patch"""
    rng = np.random.default_rng(61)
    W = (rng.random(shape) * 3.0).astype(np.float32).astype(np.float64)
    W[1:, -1, 2:4, 3:7] = 0.0
    kw = dict(reg_z_over_reg=1.3, reg_time=0.8, mask_static=W)
    x0 = _input(shape, 7)
    if n > 24:
        assert n > pytv.solvers.ChambollePock.SMALL_BLOCK            # the long case spans two launches
    _check(pytv, "cp", x0, n, scheme, kw)
    _check(pytv, "sg", x0, n + 1, scheme, kw, step=STEP_LONG if n > 24 else STEP)


# ---- 2. weight maps and mask variants, every form ---------------------------------------------------------------------------------------
def _variant(name):
    rng = np.random.default_rng(67)
    if name == "weight_map":
        shape = (4, 3, 9, 20)
        W = (rng.random(shape[2:]) * 3.0).astype(np.float32).astype(np.float64)
        W[2:5, 4:11] = 0.0
        return shape, dict(reg_z_over_reg=1.0, reg_time=1.3, mask_static=W)
    if name == "mask_factor0":                  # the reference's defaults: a boolean mask with factor_reg_static = 0 switches time off under it
        shape = (3, 4, 10, 13)
        return shape, dict(reg_z_over_reg=0.6, reg_time=1.0, mask_static=rng.random(shape[2:]) > 0.5, factor_reg_static=0)
    if name == "mask_no_time":
        shape = (5, 2, 8, 16)
        return shape, dict(reg_z_over_reg=1.0, reg_time=0.0, mask_static=rng.random(shape[2:]) > 0.5, factor_reg_static=4.0)
    shape = (5, 3, 7, 12)                       # no_z: reg_z_over_reg = 0 with Nz > 1
    return shape, dict(reg_z_over_reg=0.0, reg_time=0.7)


@pytest.mark.parametrize("form", ["registers", "streamed2", "streamed3", "generic"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("variant", ["weight_map", "mask_factor0", "mask_no_time", "no_z"])
def test_weight_map_and_mask_variants(pytv, variant, scheme, form):
    shape, kw = _variant(variant)
    x0 = _input(shape, 9)
    with _form(form):
        _check(pytv, "cp", x0, 30, scheme, kw, what=variant + " " + form)
        _check(pytv, "sg", x0, 21, scheme, kw, what=variant + " " + form)


# ---- 3. pitched state -------------------------------------------------------------------------------------------------------------------
# ragged rows that auto_pitch pads to the 16-byte lane (fp32 Nx = 13, 70; fp64 Nx = 13: fp64 rows of 70 are whole lanes), explicit row + frame pads
PITCH_CASES = [((4, 3, 9, 13), "auto", DTYPES), ((3, 2, 6, 70), "auto", (np.float32,)),
               ((3, 2, 9, 14), (16, 9 * 16 + 8), DTYPES), ((4, 3, 7, 13), (16, 7 * 16 + 4), DTYPES)]


@pytest.mark.parametrize("form", ["registers", "streamed2", "generic"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,pitch,dtypes", PITCH_CASES)
def test_pitched_state(pytv, shape, pitch, dtypes, scheme, form):
    """a pitched row is vectorised whatever its Nx (tv_host.h rows_vectorisable): the last lane carries pad columns that must stay zero and
    must not enter the right-border stencil"""
    x0 = _input(shape, 13)
    kw = dict(reg_z_over_reg=0.7, reg_time=1.3)
    with _form(form):
        for kind, n in (("cp", 25), ("sg", 21)):
            wx, wloss = _oracle(kind, x0, n, scheme, kw)
            for dtype in dtypes:
                rtol, atol = TOL[(kind, dtype)]
                s = _solver(pytv, kind, x0, dtype, scheme, kw, pitch=pitch)
                assert s.geo.pitched
                if pitch != "auto":
                    assert s.x.stride()[-2] == pitch[0] and s.x.stride()[-3] == pitch[1]
                msg = "%s %s %s %s %s" % (kind, scheme, form, np.dtype(dtype).name, pitch)
                np.testing.assert_allclose(s.run(n), wloss, rtol=rtol, err_msg=msg)
                np.testing.assert_allclose(s.result().cpu().numpy(), wx, rtol=rtol, atol=atol, err_msg=msg)
                for name in ("x", "x_alt", "p", "q"):
                    t = getattr(s, name, None)
                    if t is not None:
                        assert _pads_zero(t), "%s: pads of %s are not zero" % (msg, name)


# ---- 4. launch boundaries ---------------------------------------------------------------------------------------------------------------
FORMS = ["registers", "streamed2", "streamed3", "streamed4", "generic"]
BOUNDARY_SHAPES = [(3, 1, 8, 12), (2, 3, 6, 10)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_runs_across_launch_boundaries(pytv, scheme, form):
    """127, 128, 129, 257 iterations: one launch short of SMALL_BLOCK, exactly one, one plus a single iteration, two plus one (fp64)"""
    with _form(form):
        for shape in BOUNDARY_SHAPES:
            x0 = _input(shape, 17)
            kw = dict(reg_z_over_reg=0.8, reg_time=1.1 if shape[1] > 1 else 0.0)
            for n in (127, 128, 129, 257):
                _check(pytv, "cp", x0, n, scheme, kw, dtypes=(np.float64,), what=form)
                _check(pytv, "sg", x0, n, scheme, kw, dtypes=(np.float64,), step=STEP_LONG, what=form)


SPLITS = [(1, 299), (100, 200), (128, 172), (129, 1)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scheme", ["hybrid", "central"])
@pytest.mark.parametrize("kind", ["cp", "sg"])
def test_split_runs_are_bit_identical(pytv, kind, scheme, form):
    """run(a) then run(b) == run(a + b) bit for bit, iterate and concatenated history: x, p, q (descent: the x / x_alt ping-pong, which swaps
    after the odd first blocks 1 and 129) carry everything from launch to launch"""
    import torch
    x0 = _input((3, 3, 10, 20), 19)
    kw = dict(reg_z_over_reg=0.9, reg_time=1.2)
    with _form(form):
        for dtype in DTYPES:
            for a, b in SPLITS:
                whole = _solver(pytv, kind, x0, dtype, scheme, kw)
                lw = whole.run(a + b)
                split = _solver(pytv, kind, x0, dtype, scheme, kw)
                ls = np.concatenate([split.run(a), split.run(b)])
                msg = "%s %s %s (%d, %d)" % (kind, form, np.dtype(dtype).name, a, b)
                assert np.array_equal(ls, lw), msg
                assert torch.equal(split.result(), whole.result()), msg
                if kind == "cp":
                    assert torch.equal(split.p, whole.p) and torch.equal(split.q, whole.q), msg


# ---- 5. non-default step parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_non_default_step_parameters(pytv, scheme, form):
    x0 = _input((4, 3, 9, 16), 23)
    kw = dict(reg_z_over_reg=1.0, reg_time=0.9)
    with _form(form):
        _check(pytv, "cp", x0, 40, scheme, kw, reg=12.0, cp_kw=dict(sigma_D=0.3, sigma_A=0.6, tau=0.05), what=form)
        _check(pytv, "sg", x0, 21, scheme, kw, reg=12.0, step=0.011, what=form)


# ---- 6. epoch wrap-around ---------------------------------------------------------------------------------------------------------------
def _u32_as_i32(u):
    u %= 1 << 32
    return u - (1 << 32) if u >= 1 << 31 else u


def _seed_epoch(solver, e):
    """the workspace as earlier launches would have left it at epoch e: every flag line's counter at e - 1, epoch word e, abort word 0"""
    import torch
    ws = solver._small_ws().view(torch.int32)
    ws[:EPOCH_WORD].view(K_MAX_SMALL_BLOCKS, K_FLAG_STRIDE)[:, 0] = _u32_as_i32(e - 1)
    ws[EPOCH_WORD] = _u32_as_i32(e)
    ws[ABORT_WORD] = 0


@pytest.mark.parametrize("form", ["registers", "streamed2", "generic"])
@pytest.mark.parametrize("shape", [(5, 3, 12, 70), (8, 4, 32, 64)])
@pytest.mark.parametrize("kind", ["cp", "sg"])
def test_epoch_counter_wraps_around(pytv, kind, shape, form):
    """the phase counters are never reset (tv_small.hip:45-51): a workspace near 2^32 wraps inside a 300-iteration run (at phase 100); the
    wrap-safe comparison of small_sync must give the run of a fresh workspace bit for bit.  (A broken comparison gives wrong numbers or a
    bounded abandon, never a hang.)"""
    import torch
    x0 = _input(shape, 29)
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    e = (1 << 32) - 100
    with _form(form):
        for scheme in ("hybrid", "central"):
            for dtype in DTYPES:
                fresh = _solver(pytv, kind, x0, dtype, scheme, kw)
                lf = fresh.run(300)
                wrap = _solver(pytv, kind, x0, dtype, scheme, kw)
                _seed_epoch(wrap, e)
                lw = wrap.run(300)
                msg = "%s %s %s %s" % (kind, scheme, form, np.dtype(dtype).name)
                assert int(wrap._small_ws().view(torch.int32)[EPOCH_WORD].item()) == _u32_as_i32(e + 600), msg      # it did wrap
                assert np.array_equal(lw, lf), msg
                assert torch.equal(wrap.result(), fresh.result()), msg


# ---- 7. non-finite numbers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["registers", "streamed2", "generic"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_nan_in_the_input_is_returned_not_raised(pytv, scheme, form):
    """one NaN voxel: the loss is NaN from the first iteration on every path, and the persistent loop returns it (as the reference does).
    The iterate's non-finite set equals that of the kernel pair (persistent=False), whose arithmetic the loop shares.
    KNOWN DIFFERENCE from the oracle (= the reference's numpy): there NaN spreads to every channel of a site (np.maximum and the division by
    a NaN norm propagate it), while the kernels project with fmax and guard 1/|Dx| with a comparison, so a site keeps its finite channels.
    The kernels' non-finite set is therefore a SUBSET of the oracle's, and where the oracle is finite the values agree."""
    shape = (4, 3, 9, 12)
    x0 = _input(shape, 31)
    x0[2, 1, 4, 5] = np.nan
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    with _form(form):
        for kind, n in (("cp", 6), ("sg", 5)):
            wx, wloss = _oracle(kind, x0, n, scheme, kw)
            assert np.all(np.isnan(wloss))
            for dtype in DTYPES:
                rtol, atol = TOL[(kind, dtype)]
                msg = "%s %s %s %s" % (kind, scheme, form, np.dtype(dtype).name)
                s = _solver(pytv, kind, x0, dtype, scheme, kw)
                loss = s.run(n)                                  # no RuntimeError
                np.testing.assert_allclose(loss, wloss, rtol=rtol, equal_nan=True, err_msg=msg)
                ref = _solver(pytv, kind, x0, dtype, scheme, kw, persistent=False)
                np.testing.assert_allclose(ref.run(n), wloss, rtol=rtol, equal_nan=True, err_msg=msg)
                got, pair = s.result().cpu().numpy(), ref.result().cpu().numpy()
                bad = ~np.isfinite(got)
                assert np.array_equal(bad, ~np.isfinite(pair)), msg
                assert bad[2, 1, 4, 5] and np.all(bad <= ~np.isfinite(wx)), msg
                fin = np.isfinite(wx)
                np.testing.assert_allclose(got[fin], wx[fin], rtol=rtol, atol=atol, err_msg=msg)


@pytest.mark.parametrize("form", ["registers", "generic"])
def test_diverging_descent_is_returned_not_raised(pytv, form):
    """fp32, step 3: x - x0 doubles every iteration until the fidelity and then x overflow (within the first launch); the persistent loop returns
    the history like the per-iteration kernels do: same finite prefix, same first non-finite iteration"""
    x0 = _input((3, 2, 9, 14), 37)
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    n = 160
    with _form(form):
        s = _solver(pytv, "sg", x0, np.float32, "hybrid", kw, step=3.0)
        loss = s.run(n)
        ref = _solver(pytv, "sg", x0, np.float32, "hybrid", kw, step=3.0, persistent=False)
        want = ref.run(n)
    bad = ~np.isfinite(want)
    assert bad.any() and not bad[0], "the descent was meant to overflow"
    first = int(np.argmax(bad))
    assert int(np.argmax(~np.isfinite(loss))) == first and not np.all(np.isfinite(loss))
    np.testing.assert_allclose(loss[:first], want[:first], rtol=1e-5)
    assert not np.all(np.isfinite(s.result().cpu().numpy()))


@pytest.mark.parametrize("form", ["registers", "generic"])
def test_abandoned_launch_raises_and_the_next_run_gets_a_zeroed_workspace(pytv, form):
    """the abort word raised by hand before the launch: every block that would wait leaves its loop, the closing reduction writes NaN, no
    block has to wait for another -- run(), run(record_loss=False) and the descent's run() must raise, and drop the workspace"""
    import torch
    x0 = _input((4, 3, 9, 16), 41)
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    with _form(form):
        for kind, calls in (("cp", (dict(), dict(record_loss=False))), ("sg", (dict(),))):
            s = _solver(pytv, kind, x0, np.float32, "hybrid", kw)
            for call in calls:
                s._small_ws().view(torch.int32)[ABORT_WORD] = 1
                with pytest.raises(RuntimeError, match="abandoned"):
                    s.run(140, **call)
                assert s._small_ws_buf is None
                ws = s._small_ws()
                assert int(ws.count_nonzero().item()) == 0
            loss = s.run(3)
            assert np.all(np.isfinite(loss)) and int(s._small_ws().view(torch.int32)[ABORT_WORD].item()) == 0
