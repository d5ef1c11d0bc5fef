"""What the Chambolle-Pock solvers on ``_ExtrapolatedCP`` hand to the library, call by call (``-m gpu``): ``solver.lib`` is replaced by a
plain Python proxy that forwards every call and notes the entry point's name and arguments.  Three ``step()`` calls and one call of the
stopping quantity (``duality_gap()`` or ``residuals()``) must produce a literal sequence of entry points, with tau / sigma / theta EQUAL (as
doubles, no tolerance) to what ``accel_schedule`` / ``cp_linear_steps`` / ``cp_step_pair`` give for that iteration on the host.

Eight classes, ``AcceleratedChambollePock``, ``HuberChambollePock`` and ``AdaptiveHuberChambollePock`` on both of their paths: eleven
configurations, fp32, schemes upwind and hybrid, shape (3, 2, 8, 64) -- the smallest that tv_cp_fused_supported accepts (Nx = 64, whole 16-byte lanes), with an interior plane, more
than one frame, unsharded.  A statement about behaviour: nothing here knows how the solvers are written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (3, 2, 8, 64)
KW = dict(reg_z_over_reg=1.0, reg_time=1.0)
REG, ALPHA, N_STEPS = 5.0, 2.0, 3
QUERIES = ("tv_cp_fused_supported", "tv_version", "tv_get_option", "tv_cp_zchunk")

# index of (tau, sigma, theta) in the argument list of each entry point that takes one (include/pytv4d.h; argument 0 is the geometry)
SCALARS = {"tv_cp_dual": dict(sigma=5), "tv_cp_dual_huber": dict(sigma=5), "tv_cp_dual_wtv": dict(sigma=6), "tv_cp_dual_vtv": dict(sigma=5),
           "tv_cp_dual_hwtv": dict(sigma=6), "tv_cp_hwtv_sweep": dict(sigma=10, tau=13, theta=14),
           "tv_cp_primal_accel": dict(tau=7, theta=8), "tv_cp_primal_prox": dict(tau=9, theta=10), "tv_cp_primal_kl": dict(tau=7, theta=8),
           "tv_cp_primal_wls": dict(tau=10, theta=11), "tv_cp_accel_sweep": dict(sigma=9, tau=11, theta=12),
           "tv_cp_huber_sweep": dict(sigma=9, tau=12, theta=13), "tv_cp_accel_fixup": dict(tau=7, theta=8)}


class Recorder:
    """forwards every attribute of the library; a call is noted as (name, args) before it is made"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def _accel_steps(S, L2):
    tau0, sigma0 = S.cp_step_pair(L2, None, None, names=("tau0", "sigma0"))
    tau, sigma, theta = S.accel_schedule(tau0, sigma0, 1.0, N_STEPS)
    return [(float(tau[k]), float(sigma[k]), float(theta[k])) for k in range(N_STEPS)]


def _linear_steps(S, L2):
    return [S.cp_linear_steps(L2, 1.0, ALPHA / REG)[:3]] * N_STEPS


G_MAX = 1.5                 # the largest of the weights ``_weights`` gives: not 1, so steps computed without it differ


def _weights(x0):
    return 0.5 + (x0 > 50).to(x0.dtype)


def _adaptive_linear_steps(S, L2):
    return [S.cp_linear_steps(L2, 1.0, ALPHA / (REG * G_MAX))[:3]] * N_STEPS


def _fixed_steps(S, L2):
    return [S.cp_step_pair(L2) + (1.0,)] * N_STEPS


# name: (class, extra constructor arguments from x0, set_fused argument or None, entry points of one step, of the stopping quantity, the
# stopping method, the host steps)
CONFIGS = {
    "accel_pair": ("AcceleratedChambollePock", lambda x0: {}, False, ["tv_cp_dual", "tv_cp_primal_accel"], ["tv_dual_gap"], "duality_gap",
                   _accel_steps),
    "accel_fused": ("AcceleratedChambollePock", lambda x0: {}, True, ["tv_cp_accel_sweep", "tv_cp_accel_fixup"], ["tv_dual_gap"], "duality_gap",
                    _accel_steps),
    "huber_pair": ("HuberChambollePock", lambda x0: dict(alpha=ALPHA), False, ["tv_cp_dual_huber", "tv_cp_primal_accel"], ["tv_dual_gap_huber"],
                   "duality_gap", _linear_steps),
    "huber_fused": ("HuberChambollePock", lambda x0: dict(alpha=ALPHA), True, ["tv_cp_huber_sweep", "tv_cp_accel_fixup"], ["tv_dual_gap_huber"],
                    "duality_gap", _linear_steps),
    "adaptive": ("AdaptiveTVChambollePock", lambda x0: dict(reg_weights=_weights(x0)), None,
                 ["tv_cp_dual_wtv", "tv_cp_primal_accel"], ["tv_dual_gap_wtv"], "duality_gap", _accel_steps),
    "vectorial": ("VectorialTVChambollePock", lambda x0: {}, None, ["tv_cp_dual_vtv", "tv_cp_primal_accel"], ["tv_dual_gap_vtv"], "duality_gap",
                  _accel_steps),
    "adaptive_huber_pair": ("AdaptiveHuberChambollePock", lambda x0: dict(reg_weights=_weights(x0), alpha=ALPHA), False,
                            ["tv_cp_dual_hwtv", "tv_cp_primal_accel"], ["tv_dual_gap_hwtv"], "duality_gap", _adaptive_linear_steps),
    "adaptive_huber_fused": ("AdaptiveHuberChambollePock", lambda x0: dict(reg_weights=_weights(x0), alpha=ALPHA), True,
                             ["tv_cp_hwtv_sweep", "tv_cp_accel_fixup"], ["tv_dual_gap_hwtv"], "duality_gap", _adaptive_linear_steps),
    "robust": ("RobustChambollePock", lambda x0: dict(fidelity="l1"), None, ["tv_cp_dual", "tv_cp_primal_prox"],
               ["tv_cp_dual_residual", "tv_cp_primal_prox"], "residuals", _fixed_steps),
    "poisson": ("PoissonChambollePock", lambda x0: {}, None, ["tv_cp_dual", "tv_cp_primal_kl"], ["tv_cp_dual_residual", "tv_cp_primal_kl"],
                "residuals", _fixed_steps),
    "weighted": ("WeightedChambollePock", lambda x0: dict(weights=(x0 > 20), lower=0.0), None, ["tv_cp_dual", "tv_cp_primal_wls"],
                 ["tv_cp_dual_residual", "tv_cp_primal_wls"], "residuals", _fixed_steps),
}


@pytest.fixture(scope="module")
def x0():
    """counts-like data in [0, 100): every class takes it (Poisson wants >= 0); computed once, never modified"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    return 100.0 * torch.rand(SHAPE, dtype=torch.float32, device="cuda", generator=gen)


@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_calls_and_step_scalars(config, scheme, x0):
    import pytv.solvers as S
    cls, extra, fused, step_names, stop_names, stop, steps = CONFIGS[config]
    solver = getattr(S, cls)(x0.clone(), REG, scheme=scheme, **extra(x0), **KW)
    rec = solver.lib = Recorder(solver.lib)
    if fused is not None:
        solver.set_fused(fused)
        assert solver.fused is fused
    x_bar_before = solver.x_bar.data_ptr()
    for _ in range(N_STEPS):
        solver.step()
    assert solver.it == N_STEPS
    stopping = getattr(solver, stop)()
    assert all(np.isfinite(v) for v in (stopping.values() if isinstance(stopping, dict) else stopping)), stopping
    calls = [(n, a) for n, a in rec.calls if n not in QUERIES]
    assert [n for n, _ in calls] == step_names * N_STEPS + stop_names

    L2 = S.normal_spectral_bound(scheme, SHAPE[0], SHAPE[1], KW["reg_z_over_reg"], KW["reg_time"])
    want = steps(S, L2)
    for k in range(N_STEPS):
        expect = dict(zip(("tau", "sigma", "theta"), want[k]))
        seen = set()
        for name, args in calls[len(step_names) * k:len(step_names) * (k + 1)]:
            for what, i in SCALARS[name].items():
                assert type(args[i]) is float and args[i] == expect[what], (k, name, what, args[i], expect[what])
                seen.add(what)
        assert seen == {"tau", "sigma", "theta"}, (k, seen)

    if fused:
        # x_bar and its partner change roles with every sweep: (A -> B), (B -> A), (A -> B); the fix-up completes what the sweep wrote
        # (xbar_in / xbar_out are arguments 1 / 8 of tv_cp_accel_sweep, tv_cp_huber_sweep and tv_cp_hwtv_sweep alike, xbar_out is 5 of the fix-up)
        sweeps, fixups = calls[0:2 * N_STEPS:2], calls[1:2 * N_STEPS:2]
        a, b = sweeps[0][1][1], sweeps[0][1][8]
        assert a == x_bar_before and b is not None and b != a
        assert [(c[1][1], c[1][8]) for c in sweeps] == [(a, b), (b, a), (a, b)]
        assert [c[1][5] for c in fixups] == [b, a, b]
        assert (solver.x_bar.data_ptr(), solver.x_bar_alt.data_ptr()) == (b, a)
    else:
        assert solver.x_bar.data_ptr() == x_bar_before


def test_adaptive_tv_refuses_the_one_sweep_path(x0):
    import pytv.solvers as S
    solver = S.AdaptiveTVChambollePock(x0.clone(), REG, torch.ones_like(x0), **KW)
    with pytest.raises(ValueError) as exc:
        solver.set_fused(True)
    assert str(exc.value) == "set_fused(True): AdaptiveTVChambollePock has no one-sweep path (the one-sweep kernels take a scalar lambda)"
    solver.set_fused(None)
    solver.set_fused(False)
    assert solver.fused is False


def test_vectorial_tv_refuses_the_one_sweep_path(x0):
    import pytv.solvers as S
    solver = S.VectorialTVChambollePock(x0.clone(), REG, **KW)
    with pytest.raises(ValueError) as exc:
        solver.set_fused(True)
    assert str(exc.value) == ("set_fused(True): VectorialTVChambollePock has no one-sweep path (the one-sweep kernels project each frame's dual "
                              "vector on its own)")
    solver.set_fused(None)
    solver.set_fused(False)
    assert solver.fused is False


def test_prox_classes_have_no_one_sweep_switch():
    import pytv.solvers as S
    for cls in (S.RobustChambollePock, S.PoissonChambollePock, S.WeightedChambollePock):
        assert not hasattr(cls, "set_fused") and not hasattr(cls, "fused"), cls
