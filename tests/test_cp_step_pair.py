"""``cp_step_pair``: the one place where the extrapolating Chambolle-Pock solvers derive and validate their step pair.  No GPU."""
import math

import pytest

L2S = (8.0, 12.0, 4 + 4 * 0.25)        # normal_spectral_bound of 2-D, 3-D and 2-D + weighted-time one-sided geometries
NAMES = (("tau", "sigma"), ("tau0", "sigma0"))


@pytest.fixture(scope="module")
def pair():
    from pytv.solvers import cp_step_pair
    return cp_step_pair


@pytest.mark.parametrize("L2", L2S)
def test_defaults_and_complements(pair, L2):
    tau, sigma = pair(L2, None, None)
    assert tau == sigma == 1.0 / math.sqrt(L2)
    assert abs(tau * sigma * L2 - 1.0) <= 1e-15
    for given in (0.01, 0.3, 1.0, 5.0):
        assert pair(L2, given, None) == (given, 1.0 / (L2 * given))
        assert pair(L2, None, given) == (1.0 / (L2 * given), given)
    assert all(type(v) is float for v in pair(L2, 1, None))


@pytest.mark.parametrize("names", NAMES)
@pytest.mark.parametrize("L2", L2S)
def test_refusals_name_the_callers_parameters(pair, L2, names):
    ok = 1.0 / math.sqrt(L2)
    for bad in (0, 0.0, -1.0, math.inf, math.nan):
        for args in ((bad, ok), (ok, bad), (bad, None), (None, bad)):
            with pytest.raises(ValueError, match=r"^%s and %s must be finite and > 0$" % names):
                pair(L2, *args, names=names)
    with pytest.raises(ValueError, match=r"^%s \* %s \* L\^2 = 1 > 1 \(L\^2 = %g: normal_spectral_bound\)" % (names + (L2,))):
        pair(L2, 1.0, (1.0 + 1e-9) / L2, names=names)
    assert pair(L2, 1.0, (1.0 + 1e-13) / L2, names=names) == (1.0, (1.0 + 1e-13) / L2)


def test_default_names_are_tau_and_sigma(pair):
    with pytest.raises(ValueError, match="^tau and sigma must"):
        pair(8.0, -1.0, None)
    with pytest.raises(ValueError, match=r"^tau \* sigma \* L\^2 = 2 > 1"):
        pair(8.0, 0.5, 0.5)
